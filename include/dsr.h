/*
 * include/dsr.h -- C-ABI of libdsr_hip.so: the MI355X (gfx950) implementation of the
 * BTK -> ASR front-end-to-decode hot path of mmdagent/distantspeechrecognition-mirror.
 *
 * Boundary rules
 *   - extern "C", opaque handles, plain pointers and sizes; no C++/torch types.
 *   - "dev" pointers are device (HBM) addresses owned by the caller; "host" pointers are
 *     ordinary host memory.  `stream` is a hipStream_t passed as void* (NULL = default).
 *   - every function returns a dsr_status: 0 = OK, otherwise 1 + the reference's
 *     error_type (btk/common/jexception.h:41-57), so JITERATOR ("end of stream",
 *     which the reference signals by exception) is DSR_E_ITERATOR.  The text of the
 *     last error on the calling thread is returned by dsr_last_error().
 *   - the library has no CPU fallback: without a usable HIP device every compute
 *     entry point fails with DSR_E_INITIALIZATION.
 *
 * Each entry point names the reference interface it replaces (file:line under
 * /root/reference).  INTEGRATION.md shows the SWIG/ctypes stubs a maintainer would add.
 */
#ifndef DSR_H
#define DSR_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int dsr_status;
enum {
  DSR_OK = 0,
  DSR_E_ERROR = 1,          /* JERROR          */
  DSR_E_ALLOCATION = 2,     /* JALLOCATION     */
  DSR_E_ARITHMETIC = 3,     /* JARITHMETIC     */
  DSR_E_CONSISTENCY = 4,    /* JCONSISTENCY    */
  DSR_E_DIMENSION = 5,      /* JDIMENSION      */
  DSR_E_INDEX = 6,          /* JINDEX          */
  DSR_E_INITIALIZATION = 7, /* JINITIALIZATION */
  DSR_E_IO = 8,             /* JIO             */
  DSR_E_ITERATOR = 9,       /* JITERATOR: end of stream */
  DSR_E_PYTHON = 10,        /* JPYTHON         */
  DSR_E_KEY = 11,           /* JKEY            */
  DSR_E_NUMERIC = 12,       /* JNUMERIC        */
  DSR_E_PARAMETER = 13,     /* JPARAMETER      */
  DSR_E_PARSE = 14,         /* JPARSE          */
  DSR_E_TYPE = 15           /* JTYPE           */
};

const char* dsr_last_error(void);
const char* dsr_version(void);
/* number of HIP devices visible; selects `device` for the calling thread */
dsr_status dsr_device_count(int* n);
dsr_status dsr_set_device(int device);
dsr_status dsr_stream_synchronize(void* stream);
/* utility for callers without their own HIP binding: synchronous device -> host copy */
dsr_status dsr_memcpy_dtoh(void* dst_host, const void* src_dev, size_t bytes, void* stream);

/* =====================================================================================
 * 1. Modulated (uniform DFT) filter banks
 *    replaces OverSampledDFTAnalysisBank / OverSampledDFTSynthesisBank
 *    (btk/modulated/modulated.h:291-321, modulated.cc:360-516, 521-674)
 * ===================================================================================== */
typedef struct dsr_fb dsr_fb;
/* prototype: m*M taps (host, double, copied as the reference copies it, modulated.cc:275-276).
   delayCompensationType 0/1/2 (modulated.cc:279-296), gainFactor as modulated.cc:444-448,660-661.
   M must be a power of two in [16, 2048] and D = M >> r >= 1. */
dsr_status dsr_fb_create(const double* prototype, int M, int m, int r, int synthesis,
                         int delayCompensationType, int gainFactor, dsr_fb** out);
void       dsr_fb_destroy(dsr_fb*);
/* frame bookkeeping of the reference (modulated.cc:461-516, 626-664) */
int dsr_fb_analysis_frames(const dsr_fb*, int nsamp);       /* ceil(n/D)-laN+processingDelay */
int dsr_fb_synthesis_blocks(const dsr_fb*, int nframes);    /* nframes-processingDelay (>=0) */
int dsr_fb_processing_delay(const dsr_fb*);
int dsr_fb_block_len(const dsr_fb*);                        /* D = M >> r */
/* Batched analysis over U utterances x C channels.
 *   x_dev     [U][C][sampStride] fp32 samples (SampleFeature with blockLen=shiftLen=D, padZeros)
 *   nsamp_dev [U] int32 valid samples per utterance
 *   X_dev     [U][C][Tmax][M/2+1] complex64 (re,im); frames t >= T_u are zero filled.
 * Only bins 0..M/2 are stored: the input is real, bin M-f is conj(bin f) (beamformer.cc:2609-2631
 * consumes exactly these). */
dsr_status dsr_fb_analysis(const dsr_fb*, const float* x_dev, const int32_t* nsamp_dev, int U, int C,
                           int64_t sampStride, int Tmax, float* X_dev, void* stream);
/* Batched synthesis.
 *   Y_dev      [U][Tmax][M/2+1] complex64, nframes_dev [U] valid frames
 *   y_dev      [U][outStride] fp32: blocks 0..nframes-pd-1 of D samples; the rest zero filled */
dsr_status dsr_fb_synthesis(const dsr_fb*, const float* Y_dev, const int32_t* nframes_dev, int U,
                            int Tmax, int64_t outStride, float* y_dev, void* stream);
/* Analysis bank and fixed-weight subband beamformer in one pass: Y_dev [U][Tmax][M/2+1] = dsr_bf_apply(dsr_fb_analysis(x)) without the channel
 * snapshots X ever being written (OverSampledDFTAnalysisBank::next per channel, modulated.cc:461-516, feeding SubbandDS / SubbandMVDR / SubbandGSC::next,
 * beamformer.cc:1137-1200,1297-1363,2583-2635, whose output is sum_c conj(w[f][c]) X_c[f] with weights that do not change from frame to frame).
 * supported(): M = 256, r = 1, m in {2, 4}, at most 16 channels, no halfBandShift, not the adapting SubbandGSCRLS; otherwise call the two steps. */
struct dsr_bf;
int        dsr_fb_analysis_beamform_supported(const dsr_fb*, const struct dsr_bf*);
dsr_status dsr_fb_analysis_beamform(const dsr_fb*, struct dsr_bf*, const float* x_dev, const int32_t* nsamp_dev, int U, int C, int64_t sampStride,
                                    int Tmax, float* Y_dev, void* stream);

/* Block-wise processing of long streams (BASELINE configs[4]: 10-minute streams handed over in 10-second blocks).  The reference operators are
 * streaming by construction: they keep ring buffers of the last m*M samples (analysis: _RealBuffer, modulated.h:79-163, modulated.cc:400-452)
 * and of the last R*m subband frames (synthesis: modulated.cc:586-664).  A dsr_fb_state carries exactly that from one call to the next
 * (m*M - D samples per (stream, channel); R*m - 1 subband frames per stream), so that the frames of all blocks together are the frames of the whole
 * stream.  All U streams advance in step: every block but a stream's last holds a multiple of D samples.
 *   analysis_block : x_dev [U][C][sampStride] the block's new samples, nsamp_dev [U]; last != 0 appends the processingDelay zero-input frames
 *                    (modulated.cc:493-501).  Frames written per stream: dsr_fb_analysis_block_frames(plan, state, nsamp, last), asked BEFORE the call
 *                    (the stream's first block spends the look-ahead of delayCompensationType 2: unless it is also the last one it must hold at
 *                    least m*R/2 - 1 blocks of D samples in every stream -- the call cannot see a shorter one, its counts are on the device, and
 *                    the frames of the stream would then come out m*R/2 - 1 blocks late).  X_dev [U][C][Tmax][M/2+1].
 *   synthesis_block: Y_dev [U][Tmax][M/2+1], nframes_dev [U] (nframesHostMax = their maximum); output blocks per stream:
 *                    dsr_fb_synthesis_block_blocks(plan, state, nframes), asked before the call (the first call keeps processingDelay frames of
 *                    look-ahead back, modulated.cc:631-634, and needs at least processingDelay + R*m frames).  y_dev [U][outStride]. */
typedef struct dsr_fb_state dsr_fb_state;
dsr_status dsr_fb_state_create(const dsr_fb*, int U, int C /* ignored for a synthesis plan */, dsr_fb_state** out);
void       dsr_fb_state_destroy(dsr_fb_state*);
dsr_status dsr_fb_state_reset(dsr_fb_state*);            /* the next block starts new streams */
int        dsr_fb_analysis_block_frames(const dsr_fb*, const dsr_fb_state*, int nsampBlock, int last);
dsr_status dsr_fb_analysis_block(const dsr_fb*, dsr_fb_state*, const float* x_dev, const int32_t* nsamp_dev, int U, int C, int64_t sampStride,
                                 int last, int Tmax, float* X_dev, void* stream);
int        dsr_fb_synthesis_block_blocks(const dsr_fb*, const dsr_fb_state*, int nframesBlock);
dsr_status dsr_fb_synthesis_block(const dsr_fb*, dsr_fb_state*, const float* Y_dev, const int32_t* nframes_dev, int nframesHostMax, int U, int Tmax,
                                  int64_t outStride, float* y_dev, void* stream);

/* =====================================================================================
 * 2. Subband beamformers
 *    replaces beamformerWeights / SubbandDS / SubbandGSC / SubbandMVDR
 *    (btk/beamformer/beamformer.h:49-118,120-223,316-383; beamformer.cc:531-594,1137-1200,
 *     1297-1447,2321-2635)
 * ===================================================================================== */
typedef struct dsr_bf dsr_bf;
dsr_status dsr_bf_create(int fftLen, int chanN, int halfBandShift, dsr_bf** out);
void       dsr_bf_destroy(dsr_bf*);
int        dsr_bf_fft_len(const dsr_bf*);
int        dsr_bf_chan_n(const dsr_bf*);
/* halfBandShift == true (beamformer.cc:544-555,1159-1175,1321-1330): all fftLen bins are computed independently -- no conjugate mirror, no special
   bin 0; the snapshot and output arrays of dsr_bf_apply then carry dsr_bf_bins() = fftLen bins per frame instead of fftLen/2+1.  Delay-and-sum and
   GSC only: SubbandMVDR refuses the flag (:2324-2327), SubbandGSCRLS::next says "not yet implemented" (:1580-1583) -- both kept. */
int        dsr_bf_half_band_shift(const dsr_bf*);
int        dsr_bf_is_adaptive(const dsr_bf*);      /* 1 after dsr_bf_rls_config: the output depends on the frames before (SubbandGSCRLS) */
int        dsr_bf_bins(const dsr_bf*);
/* calcArrayManifoldVectors (beamformer.cc:531-594): delays[chanN] seconds */
dsr_status dsr_bf_calc_array_manifold(dsr_bf*, double sampleRate, const double* delays);
/* calcDelaysPolar2 of the reference driver (btk/src/superdirectiveBeamformer.cc:118-137) */
dsr_status dsr_calc_delays_polar2(float azimuth, float elevation, const double* micPos /*[C][3]*/,
                                  int chanN, double* delays);
/* SubbandMVDR::setDiffuseNoiseModel / divideAllNonDiagonalElements / setAllLevelsOfDiagonalLoading /
   setNoiseSpatialSpectralMatrix / calcMVDRWeights (beamformer.cc:2392-2581, beamformer.h:362-378) */
dsr_status dsr_bf_set_diffuse_noise_model(dsr_bf*, const double* micPos /*[C][3]*/, double sampleRate, double sspeed);
dsr_status dsr_bf_divide_nondiagonal(dsr_bf*, float myu);
dsr_status dsr_bf_diagonal_loading(dsr_bf*, float diagonalWeight);
dsr_status dsr_bf_set_noise_matrix(dsr_bf*, int fbinX, const double* Rnn /*[C][C] complex*/);
dsr_status dsr_bf_calc_mvdr_weights(dsr_bf*, double sampleRate, double dThreshold);
/* pseudoinverse(A, invA, dThreshold) (beamformer.cc:253-305): LINPACK csvdc (btk/matrix/linpack_c.cc:9518, job 11) in complex<float>,
   V diag(1/s) U^H with singular values below dThreshold dropped.  A [rows][cols] complex128 row major (host) -> invA [cols][rows];
   *ok = the reference's return value (0: a singular value was dropped or csvdc did not converge); svals (optional) min(rows, cols) floats.
   On some exactly rank-deficient matrices (c ones(32, 32)) the reference's csvdc never returns: its deflation cases alternate and maxit counts QR
   steps only.  Here csvdc also ends after 4 maxit (n + 1) + 64 passes of any case: *ok = 0 and invA is NaN then. */
dsr_status dsr_pseudoinverse(const double* A, int rows, int cols, float dThreshold, double* invA, int* ok, float* svals);
/* SubbandGSC: calcGSCWeights (blocking matrices), setActiveWeights_f, zeroActiveWeights
   (beamformer.cc:1373-1447, 761-799, 398-479) */
dsr_status dsr_bf_calc_gsc_weights(dsr_bf*, double sampleRate, const double* delays);
dsr_status dsr_bf_set_active_weights(dsr_bf*, int fbinX, const double* packedWeight /*2*(C-1)*/);
dsr_status dsr_bf_zero_active_weights(dsr_bf*);
/* SubbandMVDRGSC (beamformer.h:394-425, beamformer.cc:2637-2817): mode 4 of dsr_bf_select = w_mvdr - wl with wl = B wa as cached by
 * the last setActiveWeights_f / zeroActiveWeights.  calcBlockingMatrix1(sampleRate, delays) is dsr_bf_calc_gsc_weights; calcBlockingMatrix2(),
 * upgradeBlockingMatrix(), blockingMatrixOutput(outChanX) for a batch (Y_dev [U][Tmax][M/2+1]) */
dsr_status dsr_bf_calc_blocking_matrix2(dsr_bf*);
dsr_status dsr_bf_upgrade_blocking_matrix(dsr_bf*);
dsr_status dsr_bf_blocking_matrix_output(dsr_bf*, const float* X_dev, int U, int Tmax, int outChanX, float* Y_dev, void* stream);
/* SubbandGSCRLS(fftLen, halfBandShift, myu, sigma2) (beamformer.h:213-262, beamformer.cc:1497-1698; SURVEY 8f rank 3, first operator): after
 * rls_config the object's apply is the GSC whose active weights follow a recursive-least-squares update after every frame; every utterance
 * of a batch starts from the precision matrices set here and zero active weights (the reference keeps adapting across reset()).
 * initPrecisionMatrix / setPrecisionMatrix / setQuadraticConstraint(alpha, qctype: 0 none, 1 constant norm, 2 threshold) /
 * updateActiveWeightVecotrs(flag) */
dsr_status dsr_bf_rls_config(dsr_bf*, float myu, float sigma2);
dsr_status dsr_bf_rls_init_precision(dsr_bf*, float sigma2);
dsr_status dsr_bf_rls_set_precision(dsr_bf*, int fbinX, const double* Pz /* [C-1][C-1] complex128 */);
dsr_status dsr_bf_rls_quadratic_constraint(dsr_bf*, float alpha, int qctype);
dsr_status dsr_bf_rls_adapt(dsr_bf*, int flag);
/* X_dev [U][C][Tmax][M/2+1] complex64 -> Y_dev [U][Tmax][M/2+1]; wa_out_dev (optional) [U][M/2+1][C-1] complex128: the final active weights.
 * nframes_dev (optional) [U]: utterance u is adapted over its first nframes[u] frames only -- the reference stops adapting at the stream's last
 * frame (beamformer.cc:1552-1612) -- and the rest of its rows is zero.  chanN <= 64. */
dsr_status dsr_bf_gsc_rls(dsr_bf*, const float* X_dev, const int32_t* nframes_dev, int U, int Tmax, float* Y_dev, double* wa_out_dev, void* stream);
/* Carried adaptation state.  The reference object keeps its precision matrices and active weights across reset() (beamformer.cc:1552-1700: only
 * initPrecisionMatrix / setPrecisionMatrix re-seed them).  carry = 1: every dsr_bf_gsc_rls / dsr_bf_apply(_frames) call of the same U continues from
 * the state the previous one left -- block-wise processing of long streams, stream u of one call = stream u of the next; rls_reset_state (and the
 * precision-matrix setters) make the next call start from P0 and zero weights again.  carry = 0 (default): every call starts afresh. */
dsr_status dsr_bf_rls_carry(dsr_bf*, int on);
dsr_status dsr_bf_rls_reset_state(dsr_bf*);
/* Which k_gsc_rls<CT, REG, CAP> dsr_bf_gsc_rls launches for chanN channels and where the adaptation state (precision matrix + active weights,
 * (n^2 + n) complex128 per (utterance, bin), n = chanN - 1) lives: path[0] = CT, the compile-time channel count (4, 6, 8; 0: run-time count),
 * path[1] = CAP, the capacity of a thread's vectors (16; 64 above 16 channels), path[2] = the residence.  lds (optional): lds[0] the bytes the 64
 * lanes' state takes, which the 150 KB gate compares (chanN <= 12 fits); lds[1] the dynamic LDS of the launch (lds[0] with the state in LDS, else 0).
 * The launch takes its decisions from the same helper.  The carried state (dsr_bf_rls_carry) has one layout whatever the residence.  The switches
 * DSR_RLS_NOREGS (no register residence) and DSR_RLS_MEMSTATE (no LDS residence), set to anything, are read on every call.  Needs no device. */
enum { DSR_RLS_STATE_REGS = 0,         /* k_gsc_rls<C, true, 16>: chanN 4, 6, 8 */
       DSR_RLS_STATE_LDS = 1,          /* k_gsc_rls<CT, false, 16> with dynamic LDS */
       DSR_RLS_STATE_MEM = 2 };        /* k_gsc_rls<CT, false, CAP> working in the state array, in place */
dsr_status dsr_bf_rls_path(int chanN, int path[3], int64_t lds[2]);
/* which weight set `apply` uses: 0 = delay-and-sum wq, 1 = MVDR, 2 = GSC (wq - B wa), 3 = GSC normalised, 4 = MVDR-GSC (w_mvdr - wl) */
dsr_status dsr_bf_select(dsr_bf*, int mode);
/* read back host copies: kind 0 = wq [fftLen][C], 1 = mvdr [fftLen/2+1][C], 2 = R [fftLen/2+1][C][C],
   3 = blocking matrix [fftLen][C][C-1], 4 = effective weights in use [fftLen/2+1][C]; complex double */
dsr_status dsr_bf_get(const dsr_bf*, int kind, double* out, size_t outDoubles);
/* Y[u][t][f] = w_f^H X[u][:][t][f], f = 0..M/2 (SubbandDS::next / SubbandMVDR::next / SubbandGSC::next) */
dsr_status dsr_bf_apply(dsr_bf*, const float* X_dev, int U, int Tmax, float* Y_dev, void* stream);
/* the same with per-utterance frame counts nframes_dev [U]: rows t >= nframes[u] are zero; an adapting (SubbandGSCRLS) object adapts on the valid frames only */
dsr_status dsr_bf_apply_frames(dsr_bf*, const float* X_dev, const int32_t* nframes_dev, int U, int Tmax, float* Y_dev, void* stream);

/* =====================================================================================
 * 2a. Maximum empirical kurtosis beamforming: the active weights of a GSC for a whole utterance
 *     replaces MEKSubbandBeamformer_pr / MEKSubbandBeamformer_nrm (btk/lib/mkBeamforming.py:31-658) with the minimisers they call:
 *     conjugate_pr (btk/minimizer/conjugate_pr.c, directional_minimize.c) and GSL's steepest_descent
 * Scope: NC = 1, one source, half spectrum (F = fftLen/2+1 bins).  create refuses halfBandShift and NC != 1 with DSR_E_ERROR (the reference prints
 * and exits), nSource != 1 with DSR_E_PARAMETER, chanN outside [2, DSR_MK_MAX_CHAN] with DSR_E_DIMENSION.
 * Every (utterance, bin) is one problem: minimise  -(E|Y|^4 - beta (E|Y|^2)^2) + alpha |wa|^2,  Y_t = (wq - B wa)^H X_t, over the frames
 * accumObservations(sFrame, eFrame, R) keeps: s with sFrame <= s < min(eFrame, nframes[u], Tmax) and s % R == 0.  All scalars fp64.  The packed
 * gradient is the derivative with respect to conj(wa): half the real gradient of the cost in the packed variables, as in the reference.
 * Reduction order (tests/mk_np.py restates it): 64 partial sums, partial p adds frames p, p + 64, ... in increasing order, a fixed binary
 * tree combines them, the sum is divided by N afterwards; |v| of a packed vector is the square root of the sequential sum of squares.
 * ===================================================================================== */
typedef struct dsr_mk dsr_mk;
#define DSR_MK_MAX_CHAN 64
#define DSR_MK_EVAL_CAP 2048              /* evaluations within one iteration after which a problem stops with DSR_MK_EXIT_EVAL_CAP */
enum { DSR_MK_PR = 0,                    /* MEKSubbandBeamformer_pr: conjugate gradient (Polak-Ribiere), weights as they are */
       DSR_MK_NRM = 1 };                 /* MEKSubbandBeamformer_nrm: steepest descent, |wa| clipped to |gamma| (gamma < 0: |wq|) */
enum { DSR_MK_EXIT_MAX_ITERATIONS = 0, DSR_MK_EXIT_GRADIENT = 1,   /* |g| < STOPTOLERANCE */
       DSR_MK_EXIT_DIFFERENCE = 2,       /* |cost before - cost| < DIFFSTOPTOLERANCE */
       DSR_MK_EXIT_NO_PROGRESS = 3,      /* GSL_ENOPROG */
       DSR_MK_EXIT_EVAL_CAP = 4,
       DSR_MK_EXIT_SKIPPED = 5 };        /* no selected frame, or a starting cost that is not finite: weights and statistics unchanged */
enum { DSR_MK_FRAMES_LDS = 0,            /* a problem's y0 and Z (16 chanN bytes a frame) are copied into LDS once */
       DSR_MK_FRAMES_STREAMED = 1 };     /* read from the scratch array at every evaluation */
dsr_status dsr_mk_create(int fftLen, int chanN, int NC, int nSource, int halfBandShift, dsr_mk** out);
void       dsr_mk_destroy(dsr_mk*);
/* the quiescent vectors and blocking matrices of a dsr_bf after dsr_bf_calc_gsc_weights (same fftLen and chanN, DSR_E_DIMENSION otherwise;
   DSR_E_ERROR before calc_gsc_weights): the weights found are then the ones dsr_bf_set_active_weights of that object applies */
dsr_status dsr_mk_set_fixed_weights_from_bf(dsr_mk*, const dsr_bf*);
/* wq [F][chanN], B [F][chanN][chanN-1] complex128 (host); B == NULL: the blocking matrices of _calcBlockingMatrix (beamformer.cc:398-479) */
dsr_status dsr_mk_set_fixed_weights(dsr_mk*, const double* wq, const double* B);
dsr_status dsr_mk_get_fixed_weights(const dsr_mk*, double* wq, double* B);      /* either may be NULL */
/* defaults of create: DSR_MK_PR, alpha 1e-2, beta 3, gamma -1; MAXITNS 40, TOLERANCE 1e-3, STOPTOLERANCE 1e-2, DIFFSTOPTOLERANCE 1e-5, STEPSIZE 0.01
   (the reference's _nrm defaults: alpha 0.1, DIFFSTOPTOLERANCE 1e-10) */
dsr_status dsr_mk_config(dsr_mk*, int kind, double alpha, double beta, double gamma);
dsr_status dsr_mk_minimizer(dsr_mk*, int maxItns, double tolerance, double stopTolerance, double diffStopTolerance, double stepSize);
/* X_dev [U][chanN][Tmax][F] complex64; nframes_dev (optional) [U]; fbinX: one bin, or -1 for every bin (the arrays keep their [U][F] shape; only
 * the problems run are read and written).  wa_dev [U][F][chanN-1] complex128; stats_dev (optional) [3][U][F] fp64: the carried prevAvgY2,
 * prevAvgY4, prevFrameN (storeStatistics :410-420).
 *   eval:     cost_dev [U][F], grad_dev [U][F][2 (chanN-1)] at wa_dev; a problem without a selected frame gets NaN
 *   estimate: wa_dev in (starting point) and out; info_dev [U][F][4] int32: iterations, evaluations (passes over the frames for a cost, a gradient
 *             or both), failed trials (_pr: retries of intermediate_point; _nrm: rejected trial points), exit reason; cost_dev [U][F] the final cost.
 *             DSR_MK_NRM: the weights come back clipped and stats_dev, when given, is updated (prevFrameN is advanced before it divides the new
 *             terms, as there); DSR_MK_PR: weights as the minimiser left them, stats_dev read only. */
dsr_status dsr_mk_eval(dsr_mk*, const float* X_dev, const int32_t* nframes_dev, int U, int Tmax, int sFrame, int eFrame, int R, int fbinX,
                       const double* wa_dev, const double* stats_dev, double* cost_dev, double* grad_dev, void* stream);
dsr_status dsr_mk_estimate(dsr_mk*, const float* X_dev, const int32_t* nframes_dev, int U, int Tmax, int sFrame, int eFrame, int R, int fbinX,
                           double* wa_dev, double* stats_dev, int32_t* info_dev, double* cost_dev, void* stream);
/* Y_dev [U][Tmax][F] = (wq - B wa[u][f])^H X[u][:][t][f] for every bin, weights rounded to fp32 as dsr_bf_apply's are */
dsr_status dsr_mk_apply(dsr_mk*, const float* X_dev, int U, int Tmax, const double* wa_dev, float* Y_dev, void* stream);
/* which k_mk_minimize<CT> runs for chanN channels and Tsel selected frames (path[0] = CT: 4, 6, 8, or 0 for the run-time count) and where the
   frames live (path[1]); lds (optional): lds[0] the frames that fit the LDS residence, lds[1] the dynamic LDS of the launch.  Needs no device.
   force_streamed(1) takes the LDS residence out for that handle. */
dsr_status dsr_mk_path(int chanN, int Tsel, int path[2], int64_t lds[2]);
dsr_status dsr_mk_force_streamed(dsr_mk*, int on);

/* =====================================================================================
 * 2a'. Maximum negentropy beamforming under a generalised Gaussian (GG) model, and the GG model's training
 *     replaces MNSubbandBeamformerGGDc_pr / MNSubbandBeamformerGGDc_nrm (btk/lib/mnBeamforming.py:33-792) and CGGaussianD / MLE4CGGaussianD
 *     (btk/lib/GGDcEst.py:24-293)
 * Scope, refusals, frame selection, array shapes, the packed gradient's convention, the reduction order and the exit reasons (DSR_MK_EXIT_*) are
 * those of section 2a; one source only (the reference allows two).  Every (utterance, bin) minimises, with the bin's shape f,
 *   -[ (log sigma2 + 1 + log pi) - beta (NgConst + log(f Sf) / f - log Bc) ] + alpha |wa|^2,   sigma2 = mean |Y|^2, Sf = mean |Y|^(2f),
 * by conjugate_pr.  The gradient's sums and divisor run over the frames with |Y| > 0 (:506-513).  normalizeWeight is the identity in both reference
 * classes (the clipping is commented out, :515-528 and :693-706): _pr and _nrm differ in the default beta only (0.5, 1.0) and gamma has no effect.
 * A problem without a selected frame, with all-zero outputs at the start or a starting cost that is not finite is DSR_MK_EXIT_SKIPPED.
 * log, exp and pow on this path are the deterministic fp64 functions of csrc/det_math.h (tests/mn_np.py restates them bit for bit):
 * at most 4 2^-53 relative for log, 4 (|f ln x| + 2) 2^-53 for pow.
 * ===================================================================================== */
typedef struct dsr_mn dsr_mn;
dsr_status dsr_mn_create(int fftLen, int chanN, int NC, int nSource, int halfBandShift, dsr_mn** out);          /* mnBeamforming.py:34-71 */
void       dsr_mn_destroy(dsr_mn*);
dsr_status dsr_mn_set_fixed_weights_from_bf(dsr_mn*, const dsr_bf*);                                            /* calcFixedWeights :266-307 */
dsr_status dsr_mn_set_fixed_weights(dsr_mn*, const double* wq, const double* B);                                /* setFixedWeights :236-264 */
dsr_status dsr_mn_get_fixed_weights(const dsr_mn*, double* wq, double* B);                                      /* getWq, getB :227-231 */
/* the GG model ggdL: shape [F] (host), each > 0 and finite (DSR_E_PARAMETER otherwise); the per-bin constants are fixConst's (GGDcEst.py:45-61) */
dsr_status dsr_mn_set_ggd(dsr_mn*, const double* shape);
dsr_status dsr_mn_get_constants(const dsr_mn*, double* Bc, double* NgConst, double* logBc);                     /* [F] each (host), any may be NULL */
/* defaults of create: alpha 1e-2, beta 0.5, gamma -1 (:432; _nrm: beta 1.0, :610); MAXITNS 40, TOLERANCE 1e-3, STOPTOLERANCE 1e-2,
   DIFFSTOPTOLERANCE 1e-5, STEPSIZE 0.2 (:537) */
dsr_status dsr_mn_config(dsr_mn*, double alpha, double beta, double gamma);
dsr_status dsr_mn_minimizer(dsr_mn*, int maxItns, double tolerance, double stopTolerance, double diffStopTolerance, double stepSize);
/* as dsr_mk_eval / dsr_mk_estimate / dsr_mk_apply without carried statistics (fun_MN, dfun_MN :331-416; estimateActiveWeights :537-599) */
dsr_status dsr_mn_eval(dsr_mn*, const float* X_dev, const int32_t* nframes_dev, int U, int Tmax, int sFrame, int eFrame, int R, int fbinX,
                       const double* wa_dev, double* cost_dev, double* grad_dev, void* stream);
dsr_status dsr_mn_estimate(dsr_mn*, const float* X_dev, const int32_t* nframes_dev, int U, int Tmax, int sFrame, int eFrame, int R, int fbinX,
                           double* wa_dev, int32_t* info_dev, double* cost_dev, void* stream);
dsr_status dsr_mn_apply(dsr_mn*, const float* X_dev, int U, int Tmax, const double* wa_dev, float* Y_dev, void* stream);
dsr_status dsr_mn_force_streamed(dsr_mn*, int on);                                                              /* dsr_mk_path names the kernel */
/* MLE4CGGaussianD.acc (GGDcEst.py:218-237) over a batch of one-channel subband samples X_dev [U][Tmax][F] complex64, nframes_dev (optional) [U],
 * with the current model p [F], sa [F] (host, each > 0).  acc [5][F] fp64 (host) = acc_in (host, may be NULL) + acc1S, acc1P, acc2P, nSample,
 * totalL.  Per sample, v2 = |X|^2: l = log v2; acc1S += exp(p l); la = l - log(Bc sa); tmp = exp(p la); acc1P += tmp la where v2 > 1e-22;
 * acc2P += tmp; totalL += (LlConst - log sa) - tmp; v2 == 0 adds to nSample and totalL only.  Order: per (utterance, bin) 64 partial sums
 * (partial q adds frames q, q + 64, ...) and a fixed binary tree, then acc_in and the utterances in increasing order: a call repeats bit for bit.
 * Zero mean only.  Returns after the stream has finished. */
dsr_status dsr_ggd_accumulate(const float* X_dev, const int32_t* nframes_dev, int U, int Tmax, int F, const double* p, const double* sa,
                              const double* acc_in, double* acc, void* stream);
/* fixConst (:45-61) for F shape parameters: B = Gamma(1/p)/Gamma(2/p), lNF, NgConst, LlConst; any output may be NULL.  Host. */
dsr_status dsr_ggd_constants(const double* p, int F, double* Bc, double* lNF, double* NgConst, double* LlConst);
/* update (:246-293) for F bins from acc [5][F]: the scaling parameter, the gradient step on p (step alpha / (1 + nItr)), both floors, the
   convergence flag |newP - p| < thresh; sigmaOnly keeps p.  A bin without a sample keeps its parameters.  Host. */
dsr_status dsr_ggd_update(const double* acc, int F, const double* p, const double* sa, int nItr, double alpha, double thresh, double floorV,
                          double floorP, int sigmaOnly, double* newSa, double* newP, int32_t* converged);
/* writeParam / readParam (:118-152): "sa p mean\nB lNF\n" with %e; out = sa, p, mean, B, lNF.  A mean that is not zero is DSR_E_PARAMETER. */
dsr_status dsr_ggd_write_param(const char* path, double sa, double p, double mean);
dsr_status dsr_ggd_read_param(const char* path, double out[5]);
/* writeAccs (:176-189): ten lines.  readAccs (:191-216) cannot run in the reference (float() of a list); its evident intent is implemented:
   a file whose nItr is not 1 is ignored (used = 0), otherwise its five statistics are added to acc. */
dsr_status dsr_ggd_write_accs(const char* path, const double acc[5], double alpha, int nItr, double thresh, double floorV, double floorP);
dsr_status dsr_ggd_read_accs(const char* path, double acc[5], int* used);
/* the deterministic fp64 log, exp and digamma of csrc/det_math.h on host arrays (test hooks; need no device) */
dsr_status dsr_det_log(const double* x, double* y, int n);
dsr_status dsr_det_exp(const double* x, double* y, int n);
dsr_status dsr_det_psi(const double* x, double* y, int n);

/* =====================================================================================
 * 2a''. The data-adaptive subband beamformers of btk/lib/subbandBeamforming.py (all line numbers below are that file's)
 *     replaces SubbandBeamformerDS (:350-436), SubbandBeamformerGSC (:549-676), SubbandBeamformerGriffithsJim (:982-1104),
 *     SubbandBeamformerMVDR (:1107-1183, sample matrix inversion) and SubbandBeamformerMPDR (:1185-1265) with the helpers they call
 * Scope: the code as shipped, one constraint (the static GSC also two), no halfBandShift, half spectrum (F = fftLen/2+1 bins; the reference's
 * MPDR loops over all fftLen bins independently, its upper half equals the conjugate mirror up to rounding).  create refuses halfBandShift and
 * any other NC with DSR_E_CONSISTENCY, chanN outside [1 + NC, DSR_ABF_MAX_CHAN] with DSR_E_DIMENSION.  All arithmetic fp64.
 * Not built: SubbandBeamformerRLS (:679-804, multiplies a C x (C-1) matrix by a C-vector at :716), SubbandBeamformerCovarSqRoot (:807-829, no
 * __iter__), SubbandBeamformerInfoSqRoot (:831-979, calls an undefined isSilence).
 * ===================================================================================== */
typedef struct dsr_abf dsr_abf;
#define DSR_ABF_MAX_CHAN 64
enum { DSR_ABF_DS = 0,                   /* SubbandBeamformerDS: conj(v) . x */
       DSR_ABF_GSC = 1,                  /* SubbandBeamformerGSC: conj(x^H wq - (x^H B) wa), wa set from outside */
       DSR_ABF_GJ = 2,                   /* SubbandBeamformerGriffithsJim: normalised LMS, silence gate, norm constraint */
       DSR_ABF_MVDR = 3,                 /* SubbandBeamformerMVDR: w = (Sx + diagLoad I)^-1 v / (v^H (Sx + diagLoad I)^-1 v) */
       DSR_ABF_MPDR = 4 };               /* SubbandBeamformerMPDR: wa = conj(L R^-1), R = B^H Sx B + diagLoad I, L = wq^H Sx B */
enum { DSR_ABF_STATE_REGS = 0,           /* state in registers (chanN 4, 6, 8), the Cholesky factor in LDS */
       DSR_ABF_STATE_LDS = 1,            /* state and factor in dynamic LDS, [entry][lane] */
       DSR_ABF_STATE_MEM = 2 };          /* state and factor in memory, [entry][utterance x bin] */
dsr_status dsr_abf_create(int kind, int fftLen, int chanN, int NC, int halfBandShift, dsr_abf** out);           /* the constructors :356, :550, :989, :1110, :1188 */
void       dsr_abf_destroy(dsr_abf*);
/* the constructor parameters of the three adaptive classes (:989-1005, :1110-1121, :1188-1198); defaults of create: beta 0.999, gamma 0.0005,
   initDiagLoad 1e10, floorSubBandSigmaK 2e7, silThresh 1e10, alpha2 0.001, staticAfter 1000; diagLoad 0.001, forgetFactor 0.99, end 20.
   diagLoad <= 0 is DSR_E_PARAMETER for MVDR / MPDR: the loaded matrix is Cholesky factorised (the reference inverts it, :1140, :1257). */
dsr_status dsr_abf_config(dsr_abf*, double beta, double gamma, double initDiagLoad, double floorSubBandSigmaK, double silThresh, double alpha2,
                          int staticAfter, double diagLoad, double forgetFactor, int end);
/* _arrayManifold and _blockingMatrix (:386-420, :603-657), bins 0..fftLen/2: wq [F][chanN], B [F][chanN][chanN-NC] complex128 (host);
   B == NULL: calcBlockingMatrix(wq[f], NC) (:249-277) */
dsr_status dsr_abf_set_fixed_weights(dsr_abf*, const double* wq, const double* B);
dsr_status dsr_abf_get_fixed_weights(const dsr_abf*, double* wq, double* B);                                      /* either may be NULL */
/* calcBlockingMatrix(vs, NC) (:249-277): B [chanN][chanN-NC]; calcNullBeamformer(w_t, w_j, NC) with getInverseMat22 (:495-546): wq [chanN];
   calcArrayManifold_f / calcArrayManifoldWoNorm_f (:438-493; normalize != 0: divided by chanN): vs [chanN].  Host, complex128, no device. */
dsr_status dsr_abf_blocking_matrix(const double* vs, int chanN, int NC, double* B);
dsr_status dsr_abf_null_beamformer(const double* w_t, const double* w_j, int chanN, int NC, double* wq);
dsr_status dsr_abf_manifold(int fbinX, int fftLen, int chanN, double sampleRate, const double* delays, int halfBandShift, int normalize, double* vs);
/* setWa (:659-676), the static GSC: wa [F][chanN-NC] complex128 (host) */
dsr_status dsr_abf_set_active_weights(dsr_abf*, const double* wa);
/* __iter__ (:363-384, :564-601, :1007-1090, :1123-1168, :1200-1238) for a batch.  X_dev [U][chanN][Tmax][F] complex64 -> Y_dev [U][Tmax][F] complex64.
 * nframes_dev (optional) [U]: utterance u has nframes[u] frames; the rest of its rows is zero and nothing adapts on them.  wp_dev (optional)
 * [U][Tmax][F] fp32: the post-filter weights _wp / wp1L, row t scales frame t of this call while t < wpFrames_dev[u] (NULL: every row).
 * wOut_dev (optional, adaptive kinds): the final weights, complex128 -- _waHK [U][F][chanN-1] (Griffiths-Jim), conj(_wH) = w [U][F][chanN]
 * (MVDR), _waK [U][F][chanN-1] (MPDR): what saveWeights pickles.  Griffiths-Jim needs dsr_abf_reset once before the first call (:1092-1104
 * create the state; iterating before nextSpkr() fails in the reference too). */
dsr_status dsr_abf_run(dsr_abf*, const float* X_dev, const int32_t* nframes_dev, int U, int Tmax, const float* wp_dev, const int32_t* wpFrames_dev,
                       float* Y_dev, double* wOut_dev, void* stream);
/* carry = 1: every run of the same U continues from the state the previous one left, frame counter, gamma and average power included (the
 * reference between two iterations without nextSpkr()); carry = 0 (default): every run starts new streams.  The carried state has one layout
 * whatever the residence.  reset is nextSpkr() (:1092-1104, :1177-1183): the next run starts new streams.  A carried state of another U is
 * DSR_E_CONSISTENCY. */
dsr_status dsr_abf_set_carry(dsr_abf*, int on);
dsr_status dsr_abf_reset(dsr_abf*);
/* Which kernel dsr_abf_run launches for an adaptive kind and chanN channels: path[0] = CT, the compile-time channel count (4, 6, 8; 0: run-time
 * count), path[1] = the capacity of a thread's vectors (16; 64 above 16 channels), path[2] = the residence.  lds (optional): lds[0] the bytes the
 * 64 lanes' state and Cholesky factor take, which the 150 KB gate compares; lds[1] the dynamic LDS of the launch.  The launch takes its decisions
 * from the same helper.  The switches DSR_ABF_NOREGS and DSR_ABF_MEMSTATE, set to anything, are read on every call.  Needs no device. */
dsr_status dsr_abf_path(int kind, int chanN, int path[3], int64_t lds[2]);

/* =====================================================================================
 * 2b. Steered-response-power direction of arrival for a linear array
 *     replaces DOAEstimatorSRPDSBLA (btk/beamformer/beamformer.h:462-560, beamformer.i:479-513,
 *     beamformer.cc:2920-3283)
 * The handle holds the estimator's settings and its steering table; the accumulators are the caller's.  The table is built by the
 * first use after create / set_search_param (_calcSteeringUnitTable :3105-3152) with the geometry and frequency range of that moment
 * and kept until the next set_search_param, as in the reference: later geometry or range changes do not rebuild it.  Table work is
 * host-side and needs no GPU.  Defaults: search (-pi/2, pi/2, 0.1) (the constructor's setSearchParam, beamformer.h:531), range
 * [1, fftLen/2], threshold 0.  Deviations: where the reference reads out of bounds (fewer positions than channels, fbinMax beyond
 * the table or fftLen/2) the call fails with DSR_E_DIMENSION; a missing geometry is DSR_E_ERROR; widthTheta <= 0, an empty grid
 * or nBest < 1 are DSR_E_PARAMETER.
 * ===================================================================================== */
typedef struct dsr_doa dsr_doa;
/* DOAEstimatorSRPDSBLA(nBest, sampleRate, fftLen) (beamformer.cc:3078-3086) over chanN channels (chanN <= 128) */
dsr_status dsr_doa_create(int nBest, int sampleRate, int fftLen, int chanN, dsr_doa** out);
void       dsr_doa_destroy(dsr_doa*);
int        dsr_doa_nbest(const dsr_doa*);
int        dsr_doa_chan_n(const dsr_doa*);
int        dsr_doa_fft_len(const dsr_doa*);
/* how many times the steering table was built (each build zeroes the reference's accumulators, :3128-3130); has_table: 1 while one is built */
unsigned   dsr_doa_table_generation(const dsr_doa*);
int        dsr_doa_has_table(const dsr_doa*);
/* setArrayGeometry(positions) (:3094-3103): n x coordinates; only x is used, through |x_c - x_0| (in seconds of travel: no speed of sound) */
dsr_status dsr_doa_set_array_geometry(dsr_doa*, const double* positions, int n);
/* setSearchParam(minTheta, maxTheta, widthTheta) (beamformer.h:531-547): swapped when minTheta > maxTheta; clears the table */
dsr_status dsr_doa_set_search_param(dsr_doa*, double minTheta, double maxTheta, double widthTheta);
/* setFrequencyRange(fbinMin, fbinMax) (beamformer.h:529) */
dsr_status dsr_doa_set_frequency_range(dsr_doa*, int fbinMin, int fbinMax);
dsr_status dsr_doa_frequency_range(const dsr_doa*, int* fbinMin, int* fbinMax);
/* setEnergyThreshold(threshold) (beamformer.h:525-527): frames whose energy is below it are not accumulated */
dsr_status dsr_doa_set_energy_threshold(dsr_doa*, float threshold);
float      dsr_doa_energy_threshold(const dsr_doa*);
/* the grid: n = (unsigned)((maxTheta - minTheta) / widthTheta + 0.5) directions (:3113), theta_k accumulated as theta += widthTheta */
dsr_status dsr_doa_theta_n(dsr_doa*, int* n);
dsr_status dsr_doa_thetas(dsr_doa*, double* out, int n);
/* setLookDirection's delays for theta (:3257-3271): delays[chanN], feed them to dsr_bf_calc_array_manifold to steer a beamformer there */
dsr_status dsr_doa_look_delays(dsr_doa*, double theta, double* delays);
/* build the steering table now (the SRP call and dsr_doa_steering build it when needed) */
dsr_status dsr_doa_build_table(dsr_doa*);
/* steering weights of direction thetaX: out [fftLen/2+1][chanN] complex128 = wq_f for the table's bins, (1, 0) at bin 0 unless the table was
   built with fbinMin = 0, zero elsewhere (:3138-3146) */
dsr_status dsr_doa_steering(dsr_doa*, int thetaX, double* out, size_t outDoubles);
/* Which k_doa_srp<TG> dsr_doa_srp launches for this handle's grid and channel count (the table is built when needed): cell[0] = TG, the 16-direction
   tiles a workgroup owns (4, 2, 1 for NT = ceil(nTheta / 16) >= 4, >= 2, 1); cell[1] = BC, the bins staged in LDS at a time (16, 8, 4, 2, 1: the
   largest whose chanN rows of BC bins, padded by one from 4 up, are at most 128); cell[2] = KS = ceil(chanN / 4), the MFMA's K steps;
   ldsBytes (optional): the dynamic LDS of the launch, chanN x 64 frames x pitch x 8.  The launch takes its decisions from the same helper.  Needs
   no device. */
dsr_status dsr_doa_srp_cell(dsr_doa*, int cell[3], int64_t* ldsBytes);
/* next() over a batch (:3188-3245).  X_dev [U][chanN][Tmax][fftLen/2+1] complex64, nframes_dev [U]; per frame t < nframes[u]:
 *   energy_dev [U][Tmax] float: calcEnergy (:3043-3074), the reference's float accumulation bit for bit
 *   rp_dev (optional) [U][Tmax][nTheta] double: the response power of every direction, written for gated frames too
 *   nbest_rp_dev [U][Tmax][nBest] double, nbest_idx_dev [U][Tmax][nBest] int32: the frame's N-best (theta index, -1 = empty rank with rp -10e10;
 *                the reference reports theta_k and 0 as its DOA); all empty when the frame is gated
 *   acc_dev [U][nTheta] double: the caller's accumulators, ADDED to with the rp of every ungated frame (carry them from block to block)
 *   Y_dev (optional) [U][Tmax][fftLen/2+1] complex64: the last direction's beamformed bins fbinMin..fbinMax (the reference's _vector)
 *   gated_dev (optional) [U][Tmax] int32: 1 where energy < threshold
 * Frames from nframes[u] on are not touched. */
dsr_status dsr_doa_srp(dsr_doa*, const float* X_dev, const int32_t* nframes_dev, int U, int Tmax, float* energy_dev, double* rp_dev,
                       double* nbest_rp_dev, int32_t* nbest_idx_dev, double* acc_dev, float* Y_dev, int32_t* gated_dev, void* stream);
/* getFinalNBestHypotheses (:2986-3025) for U utterances: acc [U][nTheta] host -> nbest_rp [U][nBest], nbest_idx [U][nBest] host (DOA = (theta_k, 0)) */
dsr_status dsr_doa_final_nbest(dsr_doa*, const double* acc, int U, double* nbest_rp, int32_t* nbest_idx);

/* =====================================================================================
 * 2c. Spherical-array (modal) beamformers and 2-D steered-response-power direction of arrival
 *     replaces EigenBeamformer, SphericalDSBeamformer, DOAEstimatorSRPEB, DOAEstimatorSRPSphDSB
 *     (btk/beamformer/modalBeamformer.h:98-311, beamformer.i:416-633, modalBeamformer.cc:37-1385)
 * One handle serves all four: kind DSR_SPH_EB (phase-mode / HMDI weights, _calcWeights :304-345) or DSR_SPH_DS (delay-and-sum modal
 * weights, :1022-1058).  It holds the settings, the geometry, the mode amplitudes, the harmonics at the sensors, the look-direction
 * weights and the (theta, phi) steering table; the accumulators are the caller's.  As in dsr_doa the table is built by the first use
 * after create / set_search_param with the frequency range of that moment, and kept until the next set_search_param.  Table work is
 * host-side and needs no GPU.  Defaults: search theta, phi in (-pi, pi) by 0.25 (DOAEstimatorSRPBase, beamformer.cc:2922-2938), range
 * [1, fftLen/2], threshold 0, look direction (0, 0), sigma2 0, weight gain 1.  Deviations: a geometry whose sensor count differs
 * from chanN, maxOrder above 8 (dim = maxOrder^2 above 64), fbinMax beyond the table or a grid whose steering table would exceed 2^27
 * entries ((fbinMax+1) x units x max(dim, chanN)) is DSR_E_DIMENSION; a missing geometry or a
 * radius of 0 is DSR_E_ERROR (the reference throws or reads a null pointer); halfBandShift, widths <= 0, an empty grid or nBest < 1 are
 * DSR_E_PARAMETER.  minTheta > maxTheta is not swapped (unlike dsr_doa, as in modalBeamformer.h:197-205).
 * ===================================================================================== */
typedef struct dsr_sph dsr_sph;
#define DSR_SPH_EB 0
#define DSR_SPH_DS 1
/* the further beamformers of the family (modalBeamformer.cc:1387-2270), section 2c': their output is dsr_sph_beams */
#define DSR_SPH_HWNC 2
#define DSR_SPH_GSC 3
#define DSR_SPH_HWNCGSC 4
#define DSR_SPH_SPATIALDS 5
#define DSR_SPH_MOEN 6
/* EigenBeamformer / DOAEstimatorSRPEB (kind EB) or SphericalDSBeamformer / DOAEstimatorSRPSphDSB (kind DS) (modalBeamformer.cc:219-246,
   :769-777, :990-995, :1177-1182) over chanN channels (<= 128); NC is beamformerWeights' number of constraints: the GSC kinds' blocking
   matrix has dim - NC columns (1 <= NC < dim, checked when the weights are first needed), the other kinds only pass it on */
dsr_status dsr_sph_create(int kind, int nBest, int sampleRate, int fftLen, int halfBandShift, int NC, int maxOrder, int normalizeWeight, int chanN, dsr_sph** out);
void       dsr_sph_destroy(dsr_sph*);
int        dsr_sph_kind(const dsr_sph*);
int        dsr_sph_nbest(const dsr_sph*);
int        dsr_sph_chan_n(const dsr_sph*);
int        dsr_sph_fft_len(const dsr_sph*);
/* dim() = maxOrder^2 (:245) */
int        dsr_sph_dim(const dsr_sph*);
int        dsr_sph_max_order(const dsr_sph*);
/* how many times the steering table was built (each build zeroes the reference's accumulators, :818-820); has_table: 1 while one is built */
unsigned   dsr_sph_table_generation(const dsr_sph*);
int        dsr_sph_has_table(const dsr_sph*);
/* bumped by every set_array_geometry / set_eigenmike_geometry / set_look_direction / set_sigma2 / set_weight_gain and by the setters of
   section 2c' (set_wng, set_active_weights_f, set_diagonal_loading, fix_terms, set_beam(0, ..), beam_pattern): the stream operators recompute
   the rest of the utterance when it moves */
unsigned   dsr_sph_settings_generation(const dsr_sph*);
/* setArrayGeometry(a, theta_s, phi_s) (:538-564): radius a in mm (SSPEED 343740 mm/s, beamformer.h:47), n = chanN sensor angles; computes the
   harmonics at the sensors (:566-601); the steering table is not rebuilt */
dsr_status dsr_sph_set_array_geometry(dsr_sph*, double a, const double* theta_s, const double* phi_s, int n);
/* setEigenMikeGeometry() (:414-536): the 32 capsules of the EigenMike, a = 42 */
dsr_status dsr_sph_set_eigenmike_geometry(dsr_sph*);
/* getArrayGeometry(type) (:639-645): type 0 theta_s, else phi_s -> out [chanN] */
dsr_status dsr_sph_array_geometry(const dsr_sph*, int type, double* out, int n);
double     dsr_sph_radius(const dsr_sph*);
/* setLookDirection(theta, phi) (:608-625), setSigma2 / setWeightGain (modalBeamformer.h:111-112): the beamformer's weights */
dsr_status dsr_sph_set_look_direction(dsr_sph*, double theta, double phi);
dsr_status dsr_sph_set_sigma2(dsr_sph*, float sigma2);
dsr_status dsr_sph_set_weight_gain(dsr_sph*, float wgain);
/* getModeAmplitudes() (:627-637, modeAmplitude :37-170): out [fftLen/2+1][maxOrder] complex128, ka = 2 pi f a fs / (fftLen SSPEED) */
dsr_status dsr_sph_mode_amplitudes(dsr_sph*, double* out, size_t outDoubles);
/* the conjugated harmonics at the sensors _sh_s (:566-601): out [dim][chanN] complex128 */
dsr_status dsr_sph_harmonics(dsr_sph*, double* out, size_t outDoubles);
/* the look direction's weights (_calcSteeringUnit :716-746): out [fftLen/2+1][dim] complex128, bin 0 the DC weights (calcDCWeights :219-233) */
dsr_status dsr_sph_look_weights(dsr_sph*, double* out, size_t outDoubles);
/* SphericalDSBeamformer::calcWNG (:997-1020): out [fftLen/2+1]; the HWNC kinds: SphericalHWNCBeamformer::calcWNG (:1397-1418) with the ratio */
dsr_status dsr_sph_calc_wng(dsr_sph*, double* out, int n);
/* setSearchParam(minTheta, maxTheta, minPhi, maxPhi, widthTheta, widthPhi) (modalBeamformer.h:197-205): no swap; clears the table */
dsr_status dsr_sph_set_search_param(dsr_sph*, double minTheta, double maxTheta, double minPhi, double maxPhi, double widthTheta, double widthPhi);
/* setFrequencyRange(fbinMin, fbinMax) (modalBeamformer.h:196) */
dsr_status dsr_sph_set_frequency_range(dsr_sph*, int fbinMin, int fbinMax);
dsr_status dsr_sph_frequency_range(const dsr_sph*, int* fbinMin, int* fbinMax);
/* setEnergyThreshold(threshold): frames whose energy is below it are not accumulated */
dsr_status dsr_sph_set_energy_threshold(dsr_sph*, float threshold);
float      dsr_sph_energy_threshold(const dsr_sph*);
/* the grid (:803-804): nTheta = (unsigned)((maxTheta - minTheta) / widthTheta + 0.5), likewise nPhi; unit = iTheta nPhi + iPhi, theta and phi
   accumulated by repeated addition (:829-832) -> theta [units], phi [units] */
dsr_status dsr_sph_grid_n(dsr_sph*, int* nTheta, int* nPhi);
dsr_status dsr_sph_grid(dsr_sph*, double* theta, double* phi, int n);
/* build the steering table now (the SRP call and dsr_sph_steering build it when needed).  Only DSR_SPH_EB and DSR_SPH_DS have one, as the
   reference's DOAEstimatorSRPEB and DOAEstimatorSRPSphDSB: for the further kinds this, dsr_sph_steering, dsr_sph_srp_path and dsr_sph_srp are
   DSR_E_ERROR (-1 from dsr_sph_srp_path) */
dsr_status dsr_sph_build_table(dsr_sph*);
/* steering weights of one unit: out [fftLen/2+1][dim] complex128 = _calcWeights for the table's bins, (1, 0) at bin 0 unless the table was built
   with fbinMin = 0, zero elsewhere (:833-841) */
dsr_status dsr_sph_steering(dsr_sph*, int unit, double* out, size_t outDoubles);
/* the SRP path dsr_sph_srp takes: 0 the fused kernel, 1 the folded table through the linear estimator's kernel; -1 on error */
int        dsr_sph_srp_path(dsr_sph*);
/* The kernel of that path for this handle (the table is built when needed): cell[0] = the path; fused: cell[1] = TG (8, 4, 2, 1 for NT =
   ceil(units / 16) >= 8, >= 4, >= 2, 1), cell[2] = DT, the 16-row eigenbeam tiles (1, 2, 4 for dim <= 16, <= 32, above) of k_sph_srp<TG, DT>;
   folded: the linear estimator's cell for the [units][chanN] table (dsr_doa_srp_cell), cell[2] = 0; cell[3] = BC, cell[4] = KS and ldsBytes
   (optional) as dsr_doa_srp_cell has them.  The launch takes its decisions from the same helpers; follows DSR_SPH_SRP_PATH.  Needs no device. */
dsr_status dsr_sph_srp_cell(dsr_sph*, int cell[5], int64_t* ldsBytes);
/* the beamformer's next() (:347-399) over a batch: X_dev [U][chanN][Tmax][fftLen/2+1] complex64, nframes_dev [U] ->
 *   Y_dev [U][Tmax][fftLen/2+1] complex64: y = w_f^H (sh_s X_f), bin 0 with the DC weights
 *   F_dev (optional) [U][Tmax][fftLen/2+1][dim] complex64: the eigenbeams (getSnapShotArray, modalBeamformer.h:126)
 * Frames from nframes[u] on are not touched. */
dsr_status dsr_sph_apply(dsr_sph*, const float* X_dev, const int32_t* nframes_dev, int U, int Tmax, float* Y_dev, float* F_dev, void* stream);
/* next() of the DOA classes (:860-950, :1284-1370) over a batch, with dsr_doa_srp's outputs and contract, units in place of theta:
 *   energy_dev [U][Tmax] float (calcEnergy, bit for bit), rp_dev (optional) [U][Tmax][units] double, nbest_rp_dev / nbest_idx_dev
 *   [U][Tmax][nBest] (unit index, -1 = empty rank with rp -10e10), acc_dev [U][units] ADDED to, Y_dev (optional) [U][Tmax][fftLen/2+1]
 *   the last unit's bins fbinMin..fbinMax, gated_dev (optional) [U][Tmax] */
dsr_status dsr_sph_srp(dsr_sph*, const float* X_dev, const int32_t* nframes_dev, int U, int Tmax, float* energy_dev, double* rp_dev,
                       double* nbest_rp_dev, int32_t* nbest_idx_dev, double* acc_dev, float* Y_dev, int32_t* gated_dev, void* stream);
/* getFinalNBestHypotheses (beamformer.cc:2986-3025) for U utterances: acc [U][units] host -> nbest_rp [U][nBest], nbest_idx [U][nBest] host */
dsr_status dsr_sph_final_nbest(dsr_sph*, const double* acc, int U, double* nbest_rp, int32_t* nbest_idx);

/* -------------------------------------------------------------------------------------
 * 2c'. The further spherical-array beamformers and the multi-beam apply
 *     replaces SphericalHWNCBeamformer, SphericalGSCBeamformer, SphericalHWNCGSCBeamformer, SphericalMOENBeamformer,
 *     SphericalSpatialDSBeamformer (modalBeamformer.h:324-500, beamformer.i:648-770, :994-1010, modalBeamformer.cc:1387-2270) and
 *     getBeamPattern (:756-787, :2068-2099)
 * Kinds of dsr_sph_create.  HWNC: the HMDI weights scaled to a white noise gain (ratio > 0: norm 2 sqrt(pi / (chanN wng)), passed through a
 * float as normalizeWeights takes it; ratio <= 0: times 16 pi^2 / (chanN maxOrder^2)); normalizeWeight is not applied.  GSC / HWNCGSC: the DS /
 * HWNC weights as the quiescent vector wq, a blocking matrix per bin 1..fftLen/2, wl = B wa from outside; the output is wq^H F at bin 0 and
 * calcOutputOfGSC (beamformer.cc:1251-1287) above: (wq - wl), with normalizeWeight divided by ||wq - wl|| dim.  A new look direction rebuilds
 * B and keeps wl as last set, as the reference.  B is _calcBlockingMatrix (beamformer.cc:398-479) of conj(wq), each column then projected
 * against wq: B^H wq = 0 (the reference passes wq itself to a routine that blocks the conjugate of its argument, so its B does not block wq).
 * SPATIALDS: sensor-domain weights of length chanN for bins 0..fftLen/2 (no DC special case, no normalizeWeight).  MOEN: sensor-domain weights CN (A^H A + l I)^+ A^H BN through the single-precision LINPACK pseudo-inverse (threshold
 * 1e-8), CN = 2 / maxOrder^2; bin 0 is (1, 0, 0, ...); after fix_terms(1) every weight is 0 (NaN with normalizeWeight), as the reference, which
 * zeroes _fixedW before it uses it (:1993-1996, :2031-2034).  Settings take effect at once (the reference: at the next setLookDirection) and
 * bump the settings generation.  Deviations: set_active_weights_f before any set_look_direction is DSR_E_ERROR, a packed length other than
 * 2 (dim - NC) or fbinX > fftLen/2 DSR_E_DIMENSION; a setter called on a kind that lacks it is DSR_E_ERROR.
 * ------------------------------------------------------------------------------------- */
/* setWNG(ratio) (modalBeamformer.h:329); a new handle has ratio 1 */
dsr_status dsr_sph_set_wng(dsr_sph*, float ratio);
/* setActiveWeights_f(fbinX, packedWeight) (:1586-1594, :1702-1710): packed [2 (dim - NC)] (re, im) pairs -> wl[fbinX] = B[fbinX] wa */
dsr_status dsr_sph_set_active_weights_f(dsr_sph*, unsigned fbinX, const double* packed, size_t n);
/* setLevelOfDiagonalLoading(fbinX, diagonalWeight) (:1923-1930), fixTerms(flag) (modalBeamformer.h:443) */
dsr_status dsr_sph_set_diagonal_loading(dsr_sph*, unsigned fbinX, float diagonalWeight);
dsr_status dsr_sph_fix_terms(dsr_sph*, int flag);
/* the GSC kinds' wl: out [fftLen/2+1][dim] complex128; the blocking matrix of one bin: out [dim][dim - NC] complex128 (bin 0: zeros) */
dsr_status dsr_sph_wl(dsr_sph*, double* out, size_t outDoubles);
dsr_status dsr_sph_blocking_matrix(dsr_sph*, unsigned fbinX, double* out, size_t outDoubles);
/* the look direction's weights of the sensor-domain kinds (SPATIALDS, MOEN): out [fftLen/2+1][chanN] complex128 (dsr_sph_look_weights is
   DSR_E_ERROR for them, this call for the modal kinds) */
dsr_status dsr_sph_sensor_weights(dsr_sph*, double* out, size_t outDoubles);
/* beam b (0 <= b < 16) points at (theta, phi); beam 0 is the look direction (set_beam(0, ..) = set_look_direction).  The GSC kinds' active weights
   apply to beam 0 only. */
dsr_status dsr_sph_set_beam(dsr_sph*, int b, double theta, double phi);
/* beams 0..n-1 from a DOA handle's N-best: nbest_idx [n] unit indices of doa's steering table (dsr_sph_srp, dsr_sph_final_nbest); an empty
   rank (-1) is DSR_E_INDEX */
dsr_status dsr_sph_set_beams_nbest(dsr_sph*, dsr_sph* doa, const int32_t* nbest_idx, int n);
/* the sensor-domain vectors the device applies: out [NB][fftLen/2+1][chanN] complex128, y = v^H x.  Modal kinds: v = S^H w_eff folded in fp64
   (w_eff the look weights, for the GSC kinds calcOutputOfGSC's); sensor-domain kinds: the weights.  1 <= NB <= 16, else DSR_E_DIMENSION; a beam
   below NB without a direction is DSR_E_ERROR.  Host only. */
dsr_status dsr_sph_beam_weights(dsr_sph*, int NB, double* out, size_t outDoubles);
/* the multi-beam apply, any kind: X_dev [U][chanN][Tmax][fftLen/2+1] complex64, nframes_dev [U] -> Y_dev [U][NB][Tmax][fftLen/2+1] complex64,
   Y[u][b][t][f] = v_{b,f}^H X[u][:,t,f] in one pass over X; rows t >= nframes[u] are written as zeros.  NB <= 4 runs on the VALU, above that on
   v_mfma_f64_16x16x4_f64 (dsr_sph_beams_path: 0 / 1; DSR_SPH_BEAMS_PATH=valu|mfma forces one, -1 for another value); a call whose VALU table
   does not fit the kernel's LDS (beams x (fftLen/2+1) > 3072) runs on the MFMA kernel too. */
dsr_status dsr_sph_beams(dsr_sph*, const float* X_dev, const int32_t* nframes_dev, int U, int Tmax, int NB, float* Y_dev, void* stream);
int        dsr_sph_beams_path(int NB);
/* The kernel of one dsr_sph_beams call with NB beams, chanN channels and `bins` = fftLen/2+1 bins: cell[0] = 0 VALU / 1 MFMA (dsr_sph_beams_path,
   and the MFMA kernel where the VALU table does not fit); VALU: cell[1] = the row instantiation (NB up to 4, then 8, 16), cell[2] = CC, the channels
   whose conj(v) is staged at a time; MFMA: cell[1] = BCT = min(8, BC of dsr_doa_srp_cell), cell[2] = KS; ldsBytes (optional): the dynamic LDS of the
   launch.  The launch takes its decisions from the same helper.  Needs no device. */
dsr_status dsr_sph_beams_cell(int NB, int chanN, int bins, int cell[3], int64_t* ldsBytes);
/* getBeamPattern(fbinX, theta, phi, minTheta, maxTheta, minPhi, maxPhi, widthTheta, widthPhi): the grid is (int)(float)((max - min) / width +
   1.5) a side, theta and phi accumulated by addition; out [nTheta][nPhi] = |wq^H SHT(p)| of a unit plane wave p on the sphere (modal kinds,
   :756-787), |sum w p| unconjugated (MOEN, :2068-2099), |w^H p| (SPATIALDS: the inherited code dots a chanN-long with a dim-long vector).  It
   sets the look direction to (theta, phi), as the reference.  Host only. */
dsr_status dsr_sph_beam_pattern_n(double minTheta, double maxTheta, double minPhi, double maxPhi, double widthTheta, double widthPhi, int* nTheta, int* nPhi);
dsr_status dsr_sph_beam_pattern(dsr_sph*, unsigned fbinX, double theta, double phi, double minTheta, double maxTheta, double minPhi, double maxPhi,
                                double widthTheta, double widthPhi, double* out, size_t outDoubles);

/* =====================================================================================
 * 2c''. Spherical-array speaker trackers and the plane-wave simulator
 *     replaces ModalDecomposition, SpatialDecomposition (btk/beamformer/tracker.h:181-211), ModalSphericalArrayTracker,
 *     SpatialSphericalArrayTracker (tracker.h:216-330) and PlaneWaveSimulator (tracker.h:335-359); beamformer.i:820-960.
 *     An iterated extended Kalman filter in square-root form follows (theta, phi) frame by frame from the subband snapshots of the
 *     EigenMike's 32 capsules (the geometry is fixed, tracker.cc:195-297).  Argument errors are DSR_E_ARG (= DSR_E_PARAMETER): another
 *     channel count, an observation longer than the kernel holds, a setV block that is not positive definite.
 *     The subband sort (tracker.h:68-73, std::sort, ties unspecified there) puts the lower bin first among equal |B|.
 * ===================================================================================== */
#define DSR_E_ARG DSR_E_PARAMETER
typedef struct dsr_trk dsr_trk;
enum { DSR_TRK_MODAL = 0, DSR_TRK_SPATIAL = 1 };
/* the decomposition (tracker.h:183 / :201: orderN, subbandsN = fftLen, a [mm], sampleRate, useSubbandsN, 0 = all fftLen/2+1) and its tracker
   (tracker.h:306 / :323: sigma2_u, sigma2_v, sigma2_init, maxLocalN) in one handle.  chanN must be 32.  2N = 2 useSubbandsN subbandLength
   (modesN = (orderN+1)^2 modal, 32 spatial) rows above dsr_trk_max_rows are refused. */
dsr_status dsr_trk_create(int kind, int orderN, int fftLen, double a, double sampleRate, int useSubbandsN, double sigma2_u, double sigma2_v, double sigma2_init,
                          int maxLocalN, int chanN, dsr_trk** out);
void       dsr_trk_destroy(dsr_trk*);
int        dsr_trk_modes_n(const dsr_trk*);            /* tracker.h:114 */
int        dsr_trk_subband_length(const dsr_trk*);     /* tracker.h:118 */
int        dsr_trk_use_subbands_n(const dsr_trk*);     /* tracker.h:117 */
int        dsr_trk_fft_len(const dsr_trk*);            /* tracker.h:116 */
/* the largest 2N the kernel's LDS (160 KB a workgroup) admits for a kind, order and number of selected bins */
int64_t    dsr_trk_max_rows(int kind, int orderN, int useSubbandsN);
/* setV(Vk, subbandX) (tracker.h:229, tracker.cc:961-981): Vk [L][L] complex128, L = subbandLength; the lower triangle is realified as written
   (entries of the lower-left block above its diagonal keep their contents), the 2L x 2L block replaced by its Cholesky factor.  Defined for one
   call per subband on a fresh tracker.  Not positive definite: DSR_E_ARG, nothing changed.  get_v: the 2L x 2L block as stored. */
dsr_status dsr_trk_set_v(dsr_trk*, const double* Vk, size_t nDoubles, unsigned subbandX);
dsr_status dsr_trk_get_v(const dsr_trk*, unsigned subbandX, double* out, size_t outDoubles);
/* setInitialPosition (tracker.h:236) / nextSpeaker (tracker.h:235, position (0.5, 0)): the position dsr_trk_init_state writes */
dsr_status dsr_trk_set_initial_position(dsr_trk*, double theta, double phi);
dsr_status dsr_trk_next_speaker(dsr_trk*);
/* the carried state: dsr_trk_state_doubles() doubles an utterance (theta, phi, K row major, frames seen, error flag), a device buffer of the
   caller.  init_state: positionOnly == 0 as nextSpeaker leaves the tracker (the handle's initial position, K = sqrt(sqrt(sigma2_init)) I: the
   root is taken twice, tracker.cc:890, :908, :928; frame count and error flag cleared); != 0 the position alone (setInitialPosition). */
int        dsr_trk_state_doubles(const dsr_trk*);
dsr_status dsr_trk_init_state(dsr_trk*, double* state_dev, int U, int positionOnly, void* stream);
/* next() for every frame of a batch (tracker.h:310 / :327, tracker.cc:1280-1345 / :1356-1436): X_dev [U][32][Tmax][fftLen/2+1] complex64 (the
   layout of dsr_fb_analysis), one workgroup an utterance, the frames in order, fp64.  pos_dev [U][Tmax][2] float32 (the reference's output),
   pos64_dev the same before rounding, info_dev [U][Tmax] int32: bits 0-7 the local iterations used, bit 8 theta was clamped to [0.01, pi - 0.01],
   bit 9 a Givens norm was zero (the reference throws there): the utterance's state is frozen and its last position repeated.  Rows beyond
   nframes[u] are 0.  The state is read and left behind, so an utterance may come in blocks. */
dsr_status dsr_trk_run(dsr_trk*, const float* X_dev, const int32_t* nframes_dev, int U, int Tmax, double* state_dev, float* pos_dev, double* pos64_dev,
                       int32_t* info_dev, void* stream);
/* _bn [fftLen/2+1][orderN+1] = 4 pi i^n b_n(ka) (tracker.cc:106-115), _sphericalComponent [modesN][32] (conjugated, tracker.cc:117-130), the
   geometry in radians (tracker.cc:195-297): complex128 / doubles */
dsr_status dsr_trk_bn(const dsr_trk*, double* out, size_t outDoubles);
dsr_status dsr_trk_sensor_harmonics(const dsr_trk*, double* out, size_t outDoubles);
dsr_status dsr_trk_geometry(double* theta_s, double* phi_s, int n);
/* the static functions (tracker.h:124, :126-128): out2 = (re, im).  harmonic is sphPlm(n, |m|, cos theta), the sign flipped for odd negative m,
   times e^{-i m phi}: the conjugate of dsr_sph_harmonics' convention */
dsr_status dsr_trk_harmonic(int order, int degree, double theta, double phi, double* out2);
dsr_status dsr_trk_harmonic_deriv_polar(int order, int degree, double theta, double phi, double* out2);
dsr_status dsr_trk_harmonic_deriv_azimuth(int order, int degree, double theta, double phi, double* out2);
dsr_status dsr_trk_modal_coefficient(unsigned order, double ka, double* out2);
/* PlaneWaveSimulator (tracker.h:337, tracker.cc:1453-1465): the coefficients of every channel for a plane wave from (theta, phi), out
   [32][fftLen/2+1] complex128, host side.  apply (tracker.cc:1474-1488): src_dev [U][Tmax][fftLen/2+1] complex64 times coef_dev
   [chanN][fftLen/2+1] complex128 -> out_dev [U][chanN][Tmax][fftLen/2+1] complex64, or with full != 0 rows of fftLen bins, bin fftLen-k the
   conjugate of bin k; frames beyond nframes[u] are 0. */
dsr_status dsr_pws_coefficients(const dsr_trk*, double theta, double phi, double* out, size_t outDoubles);
dsr_status dsr_pws_apply(const double* coef_dev, int chanN, const float* src_dev, const int32_t* nframes_dev, int U, int Tmax, int fftLen, int full, float* out_dev,
                         void* stream);

/* =====================================================================================
 * 2d. Subband acoustic echo (voice prompt) cancellation
 *     replaces NLMSAcousticEchoCancellationFeature, KalmanFilterEchoCancellationFeature, BlockKalmanFilterEchoCancellationFeature and
 *     DTDBlockKalmanFilterEchoCancellationFeature (btk/cancelVP/cancelVP.h:41-143,428-462, cancelVP.i:62-254, cancelVP.cc:35-383,1056-1198)
 * One handle serves all four.  It holds the kind, fftLen, sampleN and the parameters; the adaptive state (filter coefficients, covariances,
 * noise variances, played history, the DTD scalars) is caller-owned device memory, like the accumulators of dsr_doa_srp.  The device works
 * on the half spectrum [U][Tmax][fftLen/2+1] complex64: the reference computes bins 0..fftLen/2 and mirrors the rest (cancelVP.cc:74-77).
 * Host-side pieces (create, setters, sizes, errors) need no GPU.  Initial state: NLMS R = 0 (the reference allocates it uninitialised and
 * relies on __iter__'s reset()); Kalman sigma2_v = K = sigma2 and sigma2_u = sigma2 (cancelVP.cc:109-122); block variants sigma2_v = sigmau2,
 * K = sigmak2 I, Sigma_u = sigmau2 I, R = 0, history zero (:216-247); DTD scalars zero (:1062).  Not reproduced: the printf dumps at bin 20,
 * the DTD constructor's debug file (:1065, :1102-1107).
 * The same handle also serves InformationFilterEchoCancellationFeature and SquareRootInformationFilterEchoCancellationFeature (cancelVP.h:264-339,
 * cancelVP.i:156-222, cancelVP.cc:386-1053): kinds DSR_AEC_INFO and DSR_AEC_SQRT_INFO, made by dsr_aec_create_info.  Initial state of both:
 * R = (1, 0, ...) (:405-407), sigma2_v = sigmau2, history zero, the per-bin _EkEnergy, _SkEnergy, _snr zero; plain kind K = sigmak2 I,
 * Sigma_u = sigmau2 I, skip counter 0; square-root kind K = Sigma_u = I / sqrt(sigmau2) (inverse Cholesky factors; sigmak2 is not used, :670-677),
 * information state zero.  Kept: the floor rule of the plain kind (a residual with |E| < 0.01 leaves as E / |E|, so a residual of exactly 0 is
 * NaN in that bin, :533-535), its reset rule (a skipped (frame, bin) pair that finds 30 counted sets that bin's filter back to (1, 0, ...),
 * :550-560), the first-100-frames branch of _updateBand (:449-475).  Deviation: the reference fixes the diagonal load at the first call in the
 * process (a function-static, :610); here every handle uses its own loading.  The two agree when a process uses one loading value.
 * ===================================================================================== */
typedef struct dsr_aec dsr_aec;
#define DSR_AEC_NLMS   0
#define DSR_AEC_KALMAN 1
#define DSR_AEC_BLOCK  2
#define DSR_AEC_DTD    3
#define DSR_AEC_INFO      8   /* made by dsr_aec_create_info only: dsr_aec_create refuses every kind outside 0..3 */
#define DSR_AEC_SQRT_INFO 9
#define DSR_AEC_MAX_SAMPLE_N 32
/* fftLen = played->size() (cancelVP.cc:41): odd or non-positive is DSR_E_PARAMETER (no power of two needed).  sampleN: the taps per bin of the
   block variants (cancelVP.i:141), 1..DSR_AEC_MAX_SAMPLE_N, otherwise DSR_E_PARAMETER (a covariance above 32 x 32 does not fit a wave's
   registers and there is no slower path); NLMS and Kalman take and ignore it (they have one tap). */
dsr_status dsr_aec_create(int kind, int fftLen, int sampleN, dsr_aec** out);
/* the information filter (squareRoot 0) or its square-root form (squareRoot != 0); fftLen and sampleN as for the block variants */
dsr_status dsr_aec_create_info(int squareRoot, int fftLen, int sampleN, dsr_aec** out);
void       dsr_aec_destroy(dsr_aec*);
int        dsr_aec_kind(const dsr_aec*);
int        dsr_aec_fft_len(const dsr_aec*);
int        dsr_aec_sample_n(const dsr_aec*);
/* one setter per parameter group, defaults = the SWIG defaults; a setter of another kind is DSR_E_PARAMETER.
   NLMS (cancelVP.i:80-81): delta 100, epsilon 1e-4, threshold 100 */
dsr_status dsr_aec_set_nlms(dsr_aec*, double delta, double epsilon, double threshold);
/* Kalman (cancelVP.i:108-113): beta 0.95, sigma2 5, threshold 100 (the SWIG constructor's sigmau2 and crossCorrTh never reach the object);
   beta outside (0, 1] is DSR_E_PARAMETER */
dsr_status dsr_aec_set_kalman(dsr_aec*, double beta, double sigma2, double threshold);
/* block and DTD (cancelVP.i:140-144, :241-246): beta 0.95, sigmau2 10e-4, sigmak2 5, threshold 100, amp4play 1; DTD ignores threshold here (its
   base-class threshold is snrTh, cancelVP.cc:1061) */
dsr_status dsr_aec_set_block(dsr_aec*, double beta, double sigmau2, double sigmak2, double threshold, double amp4play);
/* DTD only (cancelVP.i:242-243): snrTh 2, engTh 100, smooth 0.9 */
dsr_status dsr_aec_set_dtd(dsr_aec*, double snrTh, double engTh, double smooth);
/* the two information kinds only (cancelVP.i:162-163): snrTh 2, engTh 100, smooth 0.9, loading 1e-2; beta, sigmau2, sigmak2 and amp4play come
   from dsr_aec_set_block, whose threshold these kinds ignore: snrTh is also the |v[0]|^2 gate (cancelVP.cc:392) */
dsr_status dsr_aec_set_info(dsr_aec*, double snrTh, double engTh, double smooth, double loading);
/* DTD and the information kinds: which frameX _updateBand sees (cancelVP.cc:1077-1087, :1158).  0 (default) = the running frame index frame0 + t, a driver that
   calls next(t); 1 = the constant -5 of a driver that iterates (`for x in aec`), which stays in the first-100-frames branch for ever */
dsr_status dsr_aec_set_frame_mode(dsr_aec*, int mode);
/* the caller's state for U utterances: bytes to allocate (0 for a bad argument), and the initial state written into it */
size_t     dsr_aec_state_bytes(const dsr_aec*, int U);
dsr_status dsr_aec_state_init(const dsr_aec*, void* state_dev, int U, void* stream);
/* next() over a batch: played_dev, recorded_dev [U][Tmax][fftLen/2+1] complex64, nframes_dev (optional) [U] -> out_dev same shape, the residual
 * E.  Frames from nframes[u] on are written as zero and do not touch the state.  state_dev: the state the call continues from and leaves
 * behind -- block-wise processing gives the bits of one call; NULL = a fresh initial state, discarded.  frame0: the index of the call's first
 * frame (DTD and the information kinds, frame mode 0).  The block variants' reset() resets nothing, so carrying the state from utterance to utterance is the reference's
 * behaviour; starting afresh is state_init.  DTD and the plain information filter: fftLen above 2046 is DSR_E_DIMENSION (one workgroup keeps a frame's per-bin scalars in LDS).
 * The square-root information filter: a Givens rotation with a zero norm (the reference's jarithmetic_error, cancelVP.cc:699-700) is recorded
 * per utterance and reported as DSR_E_ARITHMETIC after the launch, so the call waits for its kernel. */
dsr_status dsr_aec_apply(const dsr_aec*, const float* played_dev, const float* recorded_dev, const int32_t* nframes_dev, int U, int Tmax, int frame0,
                         float* out_dev, void* state_dev, void* stream);
/* read a part of the state back (synchronous): what FILTER [U][fftLen/2+1][L] complex128, K [U][fftLen/2+1][L][L] complex128, SIGMA2V
   [U][fftLen/2+1], DTD [U][3] (_EkEnergy, _SkEnergy, _snr), HISTORY [U][fftLen/2+1][L] complex128 (entry k = the scaled played sample k frames
   back); L = 1 for NLMS and Kalman (K real).  A part the kind does not have is DSR_E_PARAMETER, a short buffer DSR_E_DIMENSION. */
#define DSR_AEC_STATE_FILTER  0
#define DSR_AEC_STATE_K       1
#define DSR_AEC_STATE_SIGMA2V 2
#define DSR_AEC_STATE_DTD     3
#define DSR_AEC_STATE_HISTORY 4
/* the information kinds: BAND [U][fftLen/2+1][3] (_EkEnergy, _SkEnergy, _snr of every bin); INFO [U][fftLen/2+1][L] complex128, the
   information state of the square-root kind, whose K is the inverse Cholesky factor the reference keeps in _K_k (lower triangular); SKIPPED [U]
   the plain kind's _skippedN, RESETS [U] how often its reset rule fired since state_init.  DSR_AEC_STATE_DTD is not a part of theirs. */
#define DSR_AEC_STATE_BAND    5
#define DSR_AEC_STATE_INFO    6
#define DSR_AEC_STATE_SKIPPED 7
#define DSR_AEC_STATE_RESETS  8
dsr_status dsr_aec_state_read(const dsr_aec*, const void* state_dev, int U, int what, double* host_out, size_t outDoubles);
/* reset() of NLMS and Kalman (cancelVP.h:60, :98): the filter coefficients become zero, sigma2_v and K live on.  For the block variants it
   does nothing, as their reset() does (cancelVP.h:134-142). */
dsr_status dsr_aec_reset_filter(const dsr_aec*, void* state_dev, int U, void* stream);

/* =====================================================================================
 * 2e. Pairwise time-delay estimation: the GCC family and CCTDE
 *     replaces GCCRaw, GCCGnnSub, GCCPhat, GCCGnnSubPhat, GCCMLRRaw, GCCMLRGnnSub (btk/localization/localization.h:75-218,
 *     localization.cc:1156-1413, localization.i:94-143) and CCTDE (btk/TDEstimator/CCTDE.h:60-101, CCTDE.cc:46-342, TDEstimator.i)
 * One handle serves the six weightings.  It holds the kind, the sizes, the pair list and the parameters; for the batch entries, what the
 * reference keeps between calls (per channel: noise power and last timestamp; per pair: noise cross-spectrum, smoothed cross-spectrum,
 * correlation) is caller-owned device memory, like the state of dsr_aec_apply, so blocks of a long stream chain exactly, and one handle
 * may serve several states and streams.  The per-call entries (dsr_gcc_calculate, dsr_gcc_peak, dsr_gcc_get) are the reference's object
 * as it is: they keep one utterance's state of their own inside the handle, take and return host data, are synchronous, and like that
 * object are not for two threads at once.  Host-side pieces (create, setters, sizes, dsr_gcc_channel_delays, dsr_cctde_check) need no GPU.  Kept quirks and stated deviations: DESIGN 4.4j.
 * ===================================================================================== */
typedef struct dsr_gcc dsr_gcc;
#define DSR_GCC_RAW        0
#define DSR_GCC_GNNSUB     1
#define DSR_GCC_PHAT       2
#define DSR_GCC_GNNSUBPHAT 3
#define DSR_GCC_MLRRAW     4
#define DSR_GCC_MLRGNNSUB  5
/* GCC(sampleRate, fftLen, nChan, pairs, alpha, beta, q, interpolate, noisereduction) (localization.h:123, localization.cc:1220-1248); the
   reference's `pairs` is a count and calculate() names the channels, here the list pairs[pairsN][2] comes first.  The constructor's alpha is
   honoured (the reference's loops that apply it run over an uninitialised index).  fftLen odd, not a power of two or outside [8, 4096] is
   DSR_E_DIMENSION, a channel outside [0, chanN) DSR_E_INDEX.  noisereduction is stored and unused, as in the reference. */
dsr_status dsr_gcc_create(int kind, double sampleRate, int fftLen, int chanN, const int32_t* pairs, int pairsN, double alpha, double beta, double q,
                          int interpolate, int noisereduction, dsr_gcc** out);
void       dsr_gcc_destroy(dsr_gcc*);
/* setAlpha / getAlpha (localization.h:134-140) */
dsr_status dsr_gcc_set_alpha(dsr_gcc*, double alpha);
double     dsr_gcc_alpha(const dsr_gcc*);
/* measuring (tools/bench_gcc.py): with timing on, dsr_gcc_run records events around k_gcc_spectrum and around k_gcc_corr; kernel_ms waits for
   the last run and gives the two times in ms.  Off by default; the results do not change. */
dsr_status dsr_gcc_set_timing(dsr_gcc*, int on);
dsr_status dsr_gcc_kernel_ms(const dsr_gcc*, double* ms2);
int        dsr_gcc_fft_len(const dsr_gcc*);
int        dsr_gcc_pairs_n(const dsr_gcc*);
int        dsr_gcc_chan_n(const dsr_gcc*);
/* the caller's state for U utterances: bytes to allocate (0 for a bad argument), and the initial state (no noise estimate, last timestamps
   0.0, zero cross-spectrum, no correlation) written into it */
size_t     dsr_gcc_state_bytes(const dsr_gcc*, int U);
dsr_status dsr_gcc_state_init(const dsr_gcc*, void* state_dev, int U, void* stream);
/* The frame loop of a driver -- for every frame t < nframes[u], for every pair p: calculate(X[c1][t], c1, X[c2][t], c2, p, timestamp[t],
 * sad[t], smooth) then findMaximum(minDelay, maxDelay) (localization.cc:1263-1340).  X_dev [U][chanN][Tmax][fftLen/2+1] complex64, or
 * complex128 when xIsDouble; nframes_dev [U] (optional); sad_dev [U][Tmax] int32, non-zero = speech = "compute", zero = "learn noise";
 * timestamp_dev [U][Tmax] double.  result_dev [U][Tmax][P][3] = delay (seconds), maxCorr, ratio; valid_dev [U][Tmax][P] = 0 until the pair's
 * first speech frame (the reference's correlation is uninitialised until then), result zero there.  A non-speech frame repeats the answer
 * of the last speech frame, searched with this call's window.  corr_dev (optional) [U][Tmax][P][fftLen] the correlation of every frame,
 * xspec_dev (optional) [U][Tmax][P][fftLen/2+1] complex128 the cross-spectrum of the speech frames (the other rows are not written);
 * without it the library keeps that intermediate itself.  Frames from nframes[u] on give zeros and do not touch the state.
 * GCCGnnSub with a speech frame before any noise frame of its pair is DSR_E_ERROR (the reference dereferences NULL); the state is
 * undefined afterwards.  The delay of pair (c1, c2) is tau_c1 - tau_c2 for arrival times tau. */
dsr_status dsr_gcc_run(dsr_gcc*, const void* X_dev, int xIsDouble, const int32_t* nframes_dev, const int32_t* sad_dev, const double* timestamp_dev, int smooth,
                       double minDelay, double maxDelay, int U, int Tmax, void* state_dev, double* result_dev, int32_t* valid_dev, double* corr_dev,
                       void* xspec_dev, void* stream);
/* findMaximum(minDelay, maxDelay) (localization.cc:1297-1340) over the correlation the state carries: result_dev [U][P][3], valid_dev [U][P] */
dsr_status dsr_gcc_find_maximum(dsr_gcc*, double minDelay, double maxDelay, int U, const void* state_dev, double* result_dev, int32_t* valid_dev, void* stream);
/* getNoisePowerSpectrum(chan) [fftLen/2+1], getNoiseCrossSpectrum(pair) [fftLen/2+1] complex128, getCrossSpectrum [fftLen/2+1] complex128,
   getCrossCorrelation [fftLen] (localization.h:130-133) of utterance u (synchronous); index = channel or pair; *exists = 0 where the reference
   would hand out NULL (no noise frame yet) or uninitialised memory (no speech frame yet).  A short buffer is DSR_E_DIMENSION. */
#define DSR_GCC_STATE_NOISE_POWER 0
#define DSR_GCC_STATE_NOISE_CROSS 1
#define DSR_GCC_STATE_CROSS       2
#define DSR_GCC_STATE_CORRELATION 3
dsr_status dsr_gcc_state_read(const dsr_gcc*, const void* state_dev, int U, int what, int u, int index, double* host_out, size_t outDoubles, int32_t* exists);
/* GCC::calculate(spectralSample1, chan1, spectralSample2, chan2, pair, timestamp, sad, smooth) (localization.h:125, localization.cc:1263-1295)
   on the handle's own state: spec1, spec2 host complex128 of n1, n2 bins, of which the first fftLen/2+1 are used.  The call names the pair's
   channels, as there; the handle's pair list is neither read nor changed.  sad != 0 with n1 != fftLen is DSR_E_DIMENSION as there, fewer than
   fftLen/2+1 bins DSR_E_DIMENSION, a pair or channel out of range DSR_E_INDEX.  It runs the kernels of dsr_gcc_run with U = Tmax = 1. */
dsr_status dsr_gcc_calculate(dsr_gcc*, const double* spec1, int n1, int chan1, const double* spec2, int n2, int chan2, int pair, double timestamp, int sad, int smooth);
/* findMaximum(minDelay, maxDelay) of that state's pair -> out3 = delay, maxCorr, ratio (getPeakDelay, getPeakCorr, getRatio); *valid = 0 and
   zeros before the pair's first speech frame */
dsr_status dsr_gcc_peak(dsr_gcc*, int pair, double minDelay, double maxDelay, double* out3, int32_t* valid);
/* the getters of dsr_gcc_state_read on that state */
dsr_status dsr_gcc_get(dsr_gcc*, int what, int index, double* host_out, size_t outDoubles, int32_t* exists);
/* Host side: per-channel delays from the pair delays of dsr_gcc_run, delays[0] = 0, by least squares over the pair graph (exact for pairs
   against channel 0); a graph that does not connect every channel to channel 0 is DSR_E_PARAMETER.  Sign: pairDelays[p] = tau_c1 - tau_c2
   is what the peak of X_c1 conj(X_c2) reports, and delays[c] = tau_c - tau_0 is the time the wavefront reaches channel c after channel 0 --
   the convention of dsr_bf_calc_array_manifold (weights e^{-j omega delay}), so the result is handed to it unchanged. */
dsr_status dsr_gcc_channel_delays(const dsr_gcc*, const double* pairDelays, double* delays);
/* CCTDE's constructor checks (CCTDE.cc:65-68): nHeldMaxCC >= fftLen, and an fftLen that is not a power of two in [8, 2^22], are
   DSR_E_DIMENSION.  Up to 4096 a workgroup transforms a block pair in LDS; longer ones (allsamples() over a recording: 2^22 samples are
   4 min 22 s at 16 kHz) run in global memory, one workgroup per pair, which is meant for the odd call and not for throughput. */
dsr_status dsr_cctde_check(int fftLen, int nHeldMaxCC);
/* CCTDE::next for nItems block pairs (CCTDE.cc:146-302): a_dev, b_dev [nItems][blockLen] float, blockLen <= fftLen (zero-padded), Hann window
   getWindow(2, fftLen), phase-only cross-correlation, the nHeldMaxCC largest values -> delays_dev [nItems][nHeldMaxCC] seconds (computed
   through float as there), args_dev the lags as FFT indices (getSampleDelays; -1 = empty), values_dev the correlation values (getCCValues) */
dsr_status dsr_cctde_run(const float* a_dev, const float* b_dev, int nItems, int blockLen, int fftLen, int nHeldMaxCC, int sampleRate, double* delays_dev,
                         int32_t* args_dev, double* values_dev, void* stream);

/* =====================================================================================
 * 2f. Multichannel cross-correlation source localisation on time-domain blocks
 *     replaces SearchGridBuilder, SGB4LinearArray, SGB4CircularArray, MCCLocalizer and MCCCalculator (btk/localization/MCCLocalizer.h:55-301,
 *     MCCLocalizer.cc:10-576; delays: localization.cc:110-142).  RMCCLocalizer is not built: its next() is an empty stub there.
 * For every block of L samples a channel the localiser walks the search grid; at a grid point the channels are shifted by the point's integer
 * sample delays tau[c] = (int)(float)(fs delay[c]), R = 1/(L-D) sum_n x_n x_n^T over n in [0, L-D) with x_n[c] = block_c[n + tau[c]] (an
 * index below zero reads the block's own tail, L + index: the reference refills its sample holder from the current block before it reads
 * it), D = (size_t)(fs maxTimeDelay), and cost = log det R - sum log R_ii (<= 0; 1 - exp(cost) is the MCCC).  The maxSource smallest costs
 * are kept, the earlier grid point winning a tie.  Blocks are independent.  The grids are host code and need no GPU; units are millimetres,
 * the speed of sound is 343740.  Deviations from the reference: set_positions copies every row and measures from microphone 0;
 * a grid without geometry is DSR_E_INITIALIZATION; the circular walk takes |sin|, |cos| in its polar step and ends when the azimuth reaches
 * 2 pi (the reference's never ends); the log-determinant comes from a Cholesky factor, a non-positive pivot giving cost 0 as a zero
 * eigenvalue does there; the eigenvalues of a kept entry are its |lambda| in ascending order.
 * ===================================================================================== */
typedef struct dsr_sgb dsr_sgb;
typedef struct dsr_mcc dsr_mcc;
#define DSR_SGB_LINEAR   0
#define DSR_SGB_CIRCULAR 1
/* SGB4LinearArray / SGB4CircularArray(nChan, isFarField, samplingFreq = 16000) (MCCLocalizer.h:87,101) */
dsr_status dsr_sgb_create(int kind, int nChan, int isFarField, unsigned samplingFreq, dsr_sgb** out);
void       dsr_sgb_destroy(dsr_sgb*);
/* setDistanceBtwMicrophones(distance), setPositionsOfMicrophones(mpos [rows][3]) (linear), setRadius(radius, height) (circular); the other
   kind is DSR_E_PARAMETER, rows != nChan DSR_E_DIMENSION */
dsr_status dsr_sgb_set_distance(dsr_sgb*, float distance);
dsr_status dsr_sgb_set_positions(dsr_sgb*, const double* mpos, int rows);
dsr_status dsr_sgb_set_radius(dsr_sgb*, float radius, float height);
/* reset(), nextSearchGrid() (*more = 0: the walk is over, the position stays; a near-field grid prints the reference's "need to be
   implemented" and is over at once), getSearchPosition() -> pos3, getTimeDelays() -> delays [nChan], maxTimeDelay() (-1 without geometry) */
dsr_status dsr_sgb_reset(dsr_sgb*);
dsr_status dsr_sgb_next(dsr_sgb*, int32_t* more);
dsr_status dsr_sgb_position(const dsr_sgb*, double* pos3);
dsr_status dsr_sgb_time_delays(dsr_sgb*, double* delays);
double     dsr_sgb_max_time_delay(const dsr_sgb*);
int        dsr_sgb_chan_n(const dsr_sgb*);
int        dsr_sgb_sampling_frequency(const dsr_sgb*);
dsr_status dsr_sgb_microphone_positions(const dsr_sgb*, double* mpos);
/* the whole walk from (0, 0, 0), the handle's own position untouched: *G = number of grid points; the first min(G, maxG) rows of
   positions [.][3], delays [.][nChan] (seconds) and tau [.][nChan] (samples) are written where the pointer is not NULL.  A near-field grid is
   DSR_E_INITIALIZATION "need to be implemented", more than 65536 points DSR_E_DIMENSION. */
dsr_status dsr_sgb_enumerate(const dsr_sgb*, int maxG, int32_t* G, double* positions, double* delays, int32_t* tau);
/* what dsr_mcc_create and dsr_mcc_run refuse, without a GPU: no geometry or a near-field grid DSR_E_INITIALIZATION; nChan outside [2, 64],
   maxSource outside [1, 64] or a grid point with |tau| > D DSR_E_DIMENSION; blockLen > 0 and < 2 D DSR_E_ERROR "Data samples are
   insufficient" (MCCLocalizer.cc:324-327) */
dsr_status dsr_mcc_check(const dsr_sgb*, int maxSource, int blockLen);
/* MCCLocalizer(sgb, maxSource = 1) (MCCLocalizer.h:216): the grid is walked once, here, and its tables are kept; later changes of the
   builder do not reach the handle */
dsr_status dsr_mcc_create(const dsr_sgb*, int maxSource, dsr_mcc** out);
void       dsr_mcc_destroy(dsr_mcc*);
/* the block-length check of dsr_mcc_run on its own (host): blockLen < 2 D is DSR_E_ERROR "Data samples are insufficient" */
dsr_status dsr_mcc_check_block(const dsr_mcc*, int blockLen);
int        dsr_mcc_grid_n(const dsr_mcc*);
int        dsr_mcc_chan_n(const dsr_mcc*);
int        dsr_mcc_max_source(const dsr_mcc*);
int        dsr_mcc_max_sample_delay(const dsr_mcc*);
/* measuring (tools/bench_mcc.py): events around k_mcc_cost, k_mcc_nbest and k_mcc_eig of the last call -> ms3 */
dsr_status dsr_mcc_set_timing(dsr_mcc*, int on);
dsr_status dsr_mcc_kernel_ms(const dsr_mcc*, double* ms3);
/* next() over a batch: x_dev [U][nChan][N] fp32, B = N / blockLen blocks an utterance; block b of utterance u is valid when
 * (b + 1) blockLen <= nsamples[u] (nsamples_dev NULL: all of them).  S = maxSource, G = grid points.  Outputs, each optional:
 * valid_dev [U][B] int32; index_dev [U][B][S] grid index (-1: fewer than S grid points); cost_dev [U][B][S] (100000 for an empty entry);
 * tau_dev [U][B][S][nChan]; position_dev [U][B][S][3]; eig_dev [U][B][S][nChan]; costmap_dev [U][B][G]; R_dev [U][B][nChan][nChan] the
 * covariance of the last grid point, lower triangle, the rest zero (getR()).  An invalid block gives valid = 0 and zeros everywhere.
 * A tile of the block goes through LDS: any blockLen >= 2 D works; D so large that fewer than 64 samples fit beside the margins
 * (about 200 at 64 channels) is DSR_E_DIMENSION. */
dsr_status dsr_mcc_run(dsr_mcc*, const float* x_dev, const int32_t* nsamples_dev, int U, int N, int blockLen, int32_t* valid_dev, int32_t* index_dev, double* cost_dev,
                       int32_t* tau_dev, double* position_dev, double* eig_dev, double* costmap_dev, double* R_dev, void* stream);
/* MCCCalculator::next (MCCLocalizer.cc:535-553) over the same batch: one candidate from the caller's delays [nChan] (host, seconds),
   cost_dev [U][B] with normalizeVariance on or off, tau_host [nChan] (optional) the shifts used; |tau| > D is DSR_E_INDEX (the reference
   reads outside its buffers).  The kernels of dsr_mcc_run with G = 1.  Synchronous. */
dsr_status dsr_mcc_calc(dsr_mcc*, const float* x_dev, const int32_t* nsamples_dev, int U, int N, int blockLen, const double* delays, int normalizeVariance,
                        int32_t* valid_dev, double* cost_dev, int32_t* tau_host, double* eig_dev, double* R_dev, void* stream);
/* host side: delays[c] = tau[c] / fs in seconds, the doubles dsr_bf_calc_array_manifold takes (a candidate's tau[c] is the arrival time at
   channel c relative to the array's reference point, the sign convention of that function) */
dsr_status dsr_mcc_channel_delays(const dsr_mcc*, const int32_t* tau, double* delays);

/* =====================================================================================
 * 2g. Block convolution with an impulse response (btk/convolution/convolution.h:40-104, convolution.cc:43-290) and the FIR filter across
 *     frames of FilterFeature (btk/feature/feature.cc:3206-3313)
 *
 * kind 0, OverlapAdd(samp, impulseResponse[P], fftLen): blocks of L samples, N = fftLen or, for fftLen 0, the smallest power of two >= L+P-1
 * (at least 4, the shortest transform here).  A block is zero-padded to N, transformed, multiplied by the response's spectrum, transformed
 * back and scaled by 1/N in fp64; its first L+P-1 samples are added into the reference's fp32 buffer, float(double(buffer) + section), oldest
 * block first.  The buffer's P-1 samples beyond a block are the carried state.
 * kind 1, OverlapSave(samp, impulseResponse[P]): blocks of L samples (the caller overlaps them), L a power of two above P, N = L; sample
 * i-P of the output is sample i of the circular convolution for i = P..L-1 (the reference starts at P, not P-1), size L-P, no state.
 * One plan holds C responses: one source gives C output channels (C = 1 is the reference's object).
 * Refusals: DSR_E_DIMENSION for an N that is no power of two, below 4 or above 2^22, fftLen < L+P-1 ("Section ... inconsistent with FFT
 * length"), P >= L for OverlapSave ("Cannot have P = ... and L = ..."), L, P or C below 1; DSR_E_PARAMETER for a null response (the reference
 * dereferences it) or an unknown kind; DSR_E_CONSISTENCY for apply() or update() before set_response().
 * ===================================================================================== */
typedef struct dsr_conv dsr_conv;
dsr_status dsr_conv_create(int kind /* 0 add, 1 save */, int L, int P, int fftLen, int C, dsr_conv** out);
void       dsr_conv_destroy(dsr_conv*);
int        dsr_conv_size(const dsr_conv*);                   /* samples of an output block: L, or L-P */
int        dsr_conv_fft_len(const dsr_conv*);
/* h_host [C][P]: the spectra are computed on the host in fp64 (_setImpulseResponse, convolution.cc:60-77,192-209) */
dsr_status dsr_conv_set_response(dsr_conv*, const double* h_host);
/* OverlapSave::update (convolution.cc:282-290) for response c: delta_host is complex[L] as there, its bins 0..L/2 are added to the L/2+1
 * stored ones (the reference's loop runs on to L-1, past the end of its own vector).  Bins 0 and L/2 are multiplied by their real part alone,
 * as in next(). */
dsr_status dsr_conv_update(dsr_conv*, int c, const double* delta_host);
/* OverlapAdd's carried buffer: P-1 floats per (utterance, response), zeros at the start (reset()); 0 bytes for OverlapSave and P = 1, where
 * state_dev may be NULL */
size_t     dsr_conv_state_bytes(const dsr_conv*, int U);
dsr_status dsr_conv_state_init(const dsr_conv*, void* state_dev, int U, void* stream);
/* x_dev float [U][Tmax][L], nframes_dev int32 [U] (NULL: Tmax each) -> y_dev float [U][C][Tmax][size].  Blocks at or past nframes[u] come out
 * zero and leave the state alone; a stream run as consecutive calls with the same state_dev equals one call bit for bit. */
dsr_status dsr_conv_apply(dsr_conv*, const float* x_dev, const int32_t* nframes_dev, int U, int Tmax, void* state_dev, float* y_dev, void* stream);
/* measurement (tools/bench_conv.py): with timing on, apply brackets its launches with events; kernel_ms waits for them and gives the last
 * call's milliseconds in the transform kernel and in the fold (with the state copy) */
dsr_status dsr_conv_set_timing(dsr_conv*, int on);
dsr_status dsr_conv_kernel_ms(const dsr_conv*, double* ms2);
/* FilterFeature::next over whole utterances: y[t][c] = float(sum_{i=-o..o} a[i+o] * double(x[t-i][c])), o = (lenA-1)/2, fp64 accumulator, i
 * ascending, frames outside [0, nframes[u]) read as zero.  An even lenA is DSR_E_DIMENSION "Length of filter (%d) is not odd.".
 * frames_count: the frames the reference's operator delivers for T source frames -- T for o >= 1 and T >= o, 0 for T < o (its priming loop hits
 * the end of the source), T+1 for lenA = 1 (it pads once before it looks at its count), the last one zeros.
 * x_dev float [U][Tmax][dim] -> y_dev float [U][Tout][dim], Tout = Tmax + (lenA == 1); frames past an utterance's count are zero. */
int        dsr_fir_frames_count(int T, int lenA);
dsr_status dsr_fir_frames_run(const float* x_dev, const int32_t* nframes_dev, const double* a_host, int lenA, int U, int Tmax, int dim, float* y_dev,
                              void* stream);

/* =====================================================================================
 * 3. MFCC feature chain
 *    replaces SampleFeature(block framing) -> PreemphasisFeature -> HammingFeature -> FFTFeature ->
 *    SpectralPowerFeature -> VTLNFeature -> MelFeature -> LogFeature -> CepstralFeature ->
 *    StorageFeature -> MeanSubtractionFeature -> AdjacentFeature -> LinearTransformFeature
 *    (btk/feature/feature.cc:610-659,1154-1355,1705-2298,2398-2503,2530-2987)
 * ===================================================================================== */
typedef struct {
  int blockLen, shiftLen, padZeros;   /* SampleFeature (feature.i:526-528): 320,160,false */
  double mu;                          /* PreemphasisFeature: 0.95; <0 disables the operator */
  int fftLen, powN;                   /* 512, 257 */
  double vtlnRatio, vtlnEdge; int vtlnVersion;   /* 1.0,1.0,1; version 0 disables VTLN */
  float rate, low, up; int filterN, melVersion;  /* 16000,0,0(->rate/2),30,1 */
  double logM, logA; int sphinxFlooring;         /* 1,1,0 */
  int ncep, dctType;                  /* 13, 1 */
  int cmnMode; double devNormFactor;  /* 0 none, 1 batch, 2 run-on (feature.cc:2573-2744) */
  int delta;                          /* AdjacentFeature: 7 (0 disables) */
  int outDim;                         /* LinearTransformFeature rows; 0 disables */
} dsr_mfcc_cfg;
void dsr_mfcc_default_cfg(dsr_mfcc_cfg*);
typedef struct dsr_mfcc dsr_mfcc;
/* lda: [outDim][(2delta+1)*ncep] row major fp32 (host) or NULL when outDim == 0 */
dsr_status dsr_mfcc_create(const dsr_mfcc_cfg*, const float* lda, dsr_mfcc** out);
void       dsr_mfcc_destroy(dsr_mfcc*);
int dsr_mfcc_frames(const dsr_mfcc*, int nsamp);   /* frames the chain yields for nsamp samples */
int dsr_mfcc_out_dim(const dsr_mfcc*);
/* y_dev [U][sampStride] fp32, nsamp_dev [U]; feat_dev [U][Tmax][outDim] fp32 (rows >= T_u zero).
   stage: 0 = final, 1 = cepstra before CMN, 2 = after CMN, 3 = log-mel, 4 = power (as float) */
dsr_status dsr_mfcc_run(dsr_mfcc*, const float* y_dev, const int32_t* nsamp_dev, int U, int64_t sampStride,
                        int Tmax, int stage, float* feat_dev, void* stream);
/* Which kernel each of the three stages of dsr_mfcc_run launches for a batch of Tmax frames: paths[0] the frames kernel, paths[1] the
   mean normalisation, paths[2] splice + linear transform.  dsr_mfcc_run takes its decisions from the same helper.  The switches
   DSR_MFCC_PLAIN, DSR_CMN_PLAIN and DSR_LDA_PLAIN (set to anything: the plain kernel of the pair) are read on every call. */
enum { DSR_MFCC_FRAMES_PLAIN = 0,      /* k_mfcc_frames<fftLen> */
       DSR_MFCC_FRAMES_W = 1 };        /* k_mfcc_frames_w<fftLen, 8>: fftLen 256 / 512 and tables within 52 KB of LDS */
enum { DSR_MFCC_CMN_NONE = 0, DSR_MFCC_CMN_PLAIN = 1,   /* k_cmn */
       DSR_MFCC_CMN_LDS = 2 };         /* k_cmn_lds: batch mode, ncep <= 64, Tmax * ncep * 4 <= 64 KB */
enum { DSR_MFCC_LDA_TOO_LARGE = -1,    /* the transform does not fit the LDS of a CU: dsr_mfcc_run returns DSR_E_DIMENSION at stage 0 */
       DSR_MFCC_LDA_SPLICE = 0,        /* k_splice_lda without a transform (outDim == 0) */
       DSR_MFCC_LDA_PLAIN = 1,         /* k_splice_lda */
       DSR_MFCC_LDA_B = 2 };           /* k_splice_lda_b<8>: outDim <= 256 and the pitched transform within 52 KB of LDS */
dsr_status dsr_mfcc_paths(const dsr_mfcc*, int Tmax, int paths[3]);
/* the same from a configuration alone (no device needed); lds (optional): the bytes of LDS the four gates compare --
   k_mfcc_frames_w's tables and buffers, k_cmn_lds's cepstra, k_splice_lda_b's and k_splice_lda's transform and rows */
dsr_status dsr_mfcc_cfg_paths(const dsr_mfcc_cfg*, int Tmax, int paths[3], int64_t lds[4]);

/* =====================================================================================
 * 4. Diagonal-covariance GMM scoring
 *    replaces CodebookSetBasic / DistribSetBasic and Distrib::score
 *    (asr/gaussian/codebookBasic.cc:258-309,431-554,645-766,906-960; distribBasic.cc:32-41,103-166)
 * ===================================================================================== */
typedef struct dsr_gmm dsr_gmm;
/* K codebooks; refN[k] Gaussians (<= 256, codebookBasic.h:41); mean/ivar [G][dimN]; det [G];
   val [G] = -log w of the (1:1) distribution; scale[K] or NULL (=1).  All host pointers. */
dsr_status dsr_gmm_create(int K, int dimN, const int32_t* refN, const float* mean, const float* ivar,
                          const float* det, const float* val, const float* scale, dsr_gmm** out);
/* big-endian model files written by CodebookSetBasic::save / DistribSetBasic::save */
dsr_status dsr_gmm_load(const char* codebookFile, const char* distribFile, dsr_gmm** out);
dsr_status dsr_gmm_save(const dsr_gmm*, const char* codebookFile, const char* distribFile);
/* the older (Janus) codebook-set format: dsr_gmm_load reads it when the file does not start with CodebookMagic (CodebookSetBasic::load
   :934-957 -> CodebookBasic::loadOld :311-350; a uniform covariance type or, with -1, a count and a type per Gaussian; "Wrong covariance type."
   for anything but diagonal; the compressed mode is refused as in the reference).  save_janus = save(filename, janusFormat = true) (:352-383,962-983). */
dsr_status dsr_gmm_save_janus(const dsr_gmm*, const char* codebookFile, const char* distribFile /* may be NULL */);
void       dsr_gmm_destroy(dsr_gmm*);
int dsr_gmm_num_dists(const dsr_gmm*);
int dsr_gmm_dim(const dsr_gmm*);
/* names of the set (file order) and DistribSet::find(name) / index(key) (asr/gaussian/distribBasic.h:183-190): DSR_E_KEY when absent */
const char* dsr_gmm_dist_name(const dsr_gmm*, int distX);
const char* dsr_gmm_codebook_name(const dsr_gmm*, int cbX);
dsr_status dsr_gmm_find_dist(const dsr_gmm*, const char* name, int* distX);
/* x_dev [N][dimN] fp32 -> score_dev [N][K] fp32 (cost), argmin_dev [N][K] u8 or NULL.
   mode 0: _scoreOpt nearest Gaussian, bit-exact reference order; mode 1: _scoreAll log-sum;
   mode 2: _scoreOpt through the fp32-MFMA contraction of the expanded quadratic: argmin equals mode 0's on every frame (every codebook whose two best
   lie inside the expanded form's rounding bound is re-scored in reference order); cost within rel 2e-6 of mode 0 on well-conditioned models
   (re-scored entries: mode 0's bits), never worse than 1e-3 */
dsr_status dsr_gmm_score(dsr_gmm*, const float* x_dev, int64_t N, int mode, float* score_dev,
                         uint8_t* argmin_dev, void* stream);
/* CodebookBasic::logLhood(frame, val) (asr/gaussian/codebookBasic.cc:557-609) for every (frame, codebook): the nearest Gaussian as _scoreOpt finds it,
 * finished as that method does -- 0.5 * min, + val[argmin] when useVal (the reference's val != NULL), no codebook scale.  Bit exact (reference order). */
dsr_status dsr_gmm_log_lhood(dsr_gmm*, const float* x_dev, int64_t N, int useVal, float* score_dev, uint8_t* argmin_dev, void* stream);

/* =====================================================================================
 * 5. Static decoding graph + Viterbi token passing
 *    replaces WFSTFlyWeight (asr/decoder/wfstFlyWeight.h:47-252, .cc:63-139,299-463) and
 *    DecoderFlyWeight / _Decoder (asr/decoder/decoder.h:325-1102,1127-1139; decoder.i:147-199)
 * ===================================================================================== */
/* Lexicon (asr/dictionary/distribTree.h:40-65, distribTree.cc:36-133): symbol <-> index, indices = line order of the file (its index column is
   ignored), ';' comment lines, a repeated symbol is skipped; index() of an unknown symbol is DSR_E_KEY (List::index, btk/common/mlist.h:109-114)
   unless create != 0 */
typedef struct dsr_lexicon dsr_lexicon;
dsr_status dsr_lexicon_create(const char* name, const char* fileName /* "" or NULL: empty */, dsr_lexicon** out);
void       dsr_lexicon_destroy(dsr_lexicon*);
dsr_status dsr_lexicon_read(dsr_lexicon*, const char* fileName);
dsr_status dsr_lexicon_write(const dsr_lexicon*, const char* fileName, int writeHeader);
dsr_status dsr_lexicon_clear(dsr_lexicon*);
int        dsr_lexicon_size(const dsr_lexicon*);
const char* dsr_lexicon_name(const dsr_lexicon*);
int        dsr_lexicon_is_present(const dsr_lexicon*, const char* symbol);
dsr_status dsr_lexicon_index(dsr_lexicon*, const char* symbol, int create, unsigned* index);
dsr_status dsr_lexicon_symbol(const dsr_lexicon*, unsigned index, const char** symbol /* borrowed */);

typedef struct dsr_wfst dsr_wfst;
dsr_status dsr_wfst_create(dsr_wfst** out);
/* WFSTFlyWeight(statelex, inlex, outlex) (decoder.i:52-70): borrowed lexica; the text reader looks fields that are not numbers up in them
   (wfstFlyWeight.cc:311-347); inputLexicon() / outputLexicon() / stateLexicon(); hasFinalState() */
dsr_status dsr_wfst_set_lexicons(dsr_wfst*, dsr_lexicon* stateLex, dsr_lexicon* inputLex, dsr_lexicon* outputLex);
dsr_lexicon* dsr_wfst_state_lexicon(const dsr_wfst*);
dsr_lexicon* dsr_wfst_input_lexicon(const dsr_wfst*);
dsr_lexicon* dsr_wfst_output_lexicon(const dsr_wfst*);
int        dsr_wfst_has_final_state(const dsr_wfst*);
/* WFSTFlyWeightSortedOutput (asr/decoder/wfstFlyWeight.h:403-424, Node::_addEdgeForce wfstFlyWeight.cc:754-776): every node keeps its arcs ordered by
 * (output, input), a new arc in front of the first one that is not smaller.  The container DecoderWordTrace takes.  Call on an empty transducer. */
dsr_status dsr_wfst_set_sorted_output(dsr_wfst*, int on);
void       dsr_wfst_destroy(dsr_wfst*);
dsr_status dsr_wfst_read(dsr_wfst*, const char* fileName, int binary);    /* WFSTFlyWeight::read */
/* the dynamic container's text reader, WFSTransducer::read(fileName, noSelfLoops) (asr/fsm/fsm.cc:901-986): same node/arc
   order as the fly-weight reader; noSelfLoops != 0 skips every self loop (:945).  Graph for Decoder (decoder.h:1107-1125). */
dsr_status dsr_wfst_read_dynamic(dsr_wfst*, const char* fileName, int noSelfLoops);
dsr_status dsr_wfst_write(const dsr_wfst*, const char* fileName, int binary);
/* WFSTFlyWeight::write(fileName, binary, useSymbols) (asr/decoder/wfstFlyWeight.cc:415-463): useSymbols != 0 writes every arc through the lexica set with
 * dsr_wfst_set_lexicons (Edge::write :499-516: "%25s  %25s  %10s  %20s" with a non-empty state lexicon, "%10d  %10d  %10s  %20s" without; a cost below
 * 1e-4 in magnitude is left out); final-state lines -- and, with binary, the end marker -- stay numeric, as the reference writes them.  DSR_E_KEY without lexica. */
dsr_status dsr_wfst_write_symbols(const dsr_wfst*, const char* fileName, int binary, int useSymbols);
/* WFSTFlyWeight::reverse(wfst) (asr/decoder/wfstFlyWeight.cc:141-213): dst becomes src with every arc turned round -- a super-initial node (index
 * _MaximumIndex - 3 = 536870908) with an epsilon arc to each of src's final nodes carrying that node's cost, src's initial state as the only final node.
 * WFSTFlyWeight::reverseRead(fileName) (:215-297): the same from a text file (its first arc's source becomes the final node; a final-state line must come
 * after the arcs that mention the state: DSR_E_KEY "No state %u exists." otherwise, as the reference's find() without create). */
dsr_status dsr_wfst_reverse(dsr_wfst* dst, const dsr_wfst* src);
dsr_status dsr_wfst_reverse_read(dsr_wfst*, const char* fileName);
dsr_status dsr_wfst_add_arc(dsr_wfst*, unsigned s1, unsigned s2, unsigned input, unsigned output, float cost);
dsr_status dsr_wfst_add_final(dsr_wfst*, unsigned state, float cost);
int dsr_wfst_num_nodes(const dsr_wfst*);
int dsr_wfst_num_arcs(const dsr_wfst*);
/* iteration-order export (node 0 = initial; arcs CSR in the order Node::Iterator visits them) */
dsr_status dsr_wfst_export(const dsr_wfst*, uint32_t* nodeState, int32_t* nodeFinal, float* nodeCost,
                           int32_t* arcOff, int32_t* arcDst, uint32_t* arcIn, uint32_t* arcOut, float* arcCost);

typedef struct {
  double beam, lmScale, lmPenalty, silPenalty;   /* decoder.i:191-199: 100, 12, 0, 0 */
  uint32_t silenceX;        /* input-lexicon index of silSymbol (decoder.h:740-745) */
  int maxActive;            /* token capacity per frame  (0 = default 65536)  */
  int maxCandidates;        /* placements per frame      (0 = default 8*maxActive) */
  int64_t arenaTokens;      /* back-pointer records per utterance (0 = default 64 * frames * 1024) */
  int streams;              /* concurrent utterance slots (0 = default 2 per CU) */
  int topN;                 /* decoder.i:198 (default 0).  > 0: _processFrame expands the topN best tokens of the list, in the order of their scores
                               (SortedIterator, decoder.h:298-320; ties in list order, which std::sort leaves open) and applies no beam (:571-581) */
  int64_t latticeTokens;    /* generateLattice (decoder.i:199): > 0 keeps every placement of every frame, at most this many per utterance, for
                               dsr_decoder_lattice(); 0 (default here; the reference always builds its 'worse' chains, decoder.h:1113-1114) = 1-best only */
  /* DecoderWordTrace (asr/decoder/decoder.h:1146-1304, decoder.cc:126-470; decoder.i:201-260), wordTrace != 0: the search over a WFSTFlyWeightSortedOutput
   * whose tokens carry word traces instead of back pointers (float scores compared after rounding, decoder.cc:213-267; the end expansion's float final
   * costs, :185-201).  Results: score / ac / lm / finalStatesN / activeHypos as usual; arcs_out holds the best token's own arc (bestHypo walks prev(), which
   * these tokens do not have: one symbol); words_out / nWords the words along its word traces.  wordTraceLattice = the reference's generateLattice
   * (default 1, as in the reference): that search dereferences a null word trace in the shipped code (:239) and is refused at decode (DSR_E_CONSISTENCY);
   * set it to 0 for the 1-best search.  propagateN / fastHash only steer the refused merge and are kept for the signature; insertSilence: :414-416;
   * wordTraces: word-trace records per utterance (0 = 2^20). */
  int wordTrace, propagateN, fastHash, insertSilence, wordTraceLattice;
  int64_t wordTraces;
} dsr_decoder_cfg;
void dsr_decoder_default_cfg(dsr_decoder_cfg*);
typedef struct dsr_decoder dsr_decoder;
dsr_status dsr_decoder_create(const dsr_decoder_cfg*, dsr_decoder** out);
void       dsr_decoder_destroy(dsr_decoder*);
dsr_status dsr_decoder_set(dsr_decoder*, const dsr_wfst*);               /* DecoderFlyWeight::set */
dsr_status dsr_decoder_set_beam(dsr_decoder*, double beam);
/* _Decoder::setTokenMemoryLimit(limit) (asr/decoder/decoder.h:396) caps the reference's Token memory pool.  Tokens here live in per-slot arrays sized by
 * dsr_decoder_cfg (maxActive, maxCandidates, arenaTokens); an utterance that outgrows them gets DSR_E_ALLOCATION in its result.  There is no pool to
 * limit: the value is accepted and kept (dsr_decoder_token_memory_limit) so that drivers that set it run unchanged. */
dsr_status dsr_decoder_set_token_memory_limit(dsr_decoder*, unsigned limit);
unsigned   dsr_decoder_token_memory_limit(const dsr_decoder*);
/* DecoderFlyWeight::set(wfst) with the symbol look-ups of _Decoder::_set (decoder.h:740-745): silSymbol in the input lexicon (-> cfg.silenceX),
   eosSymbol in the output lexicon; a missing symbol is DSR_E_KEY as in the reference.  NULL symbols are not looked up. */
dsr_status dsr_decoder_set_symbols(dsr_decoder*, const dsr_wfst*, const char* silSymbol, const char* eosSymbol);
uint32_t   dsr_decoder_eos_index(const dsr_decoder*);
/* Results of the last collected decode, utterance u of its batch (the decode must have been collected with paths):
 *   best_hypo  bestHypo(useInputSymbols) (decoder.h:748-773): output symbols != 0 along the best path, or the input symbols != 0 with repetitions
 *              dropped as the reference drops them (walking from the path's end: a symbol is kept when it differs from the one kept after it),
 *              every symbol followed by one blank;
 *   best_path  bestPath() (decoder.h:775-797): the names of the distributions along the path = input symbols != 0, one per line; *count = how many;
 *   path_ids   the same sequences as ids (which 0 outputs, 1 inputs as bestHypo(true), 2 inputs as bestPath) -- no lexicon needed;
 *   final_states_n  finalStatesN() (:598-608);   trace_back_succeeded  traceBackSucceeded() (:611-637).
 * buf may be NULL to ask for the size (*need, including the terminating NUL). */
dsr_status dsr_decoder_best_hypo(const dsr_decoder*, int u, int useInputSymbols, char* buf, size_t cap, size_t* need);
dsr_status dsr_decoder_best_path(const dsr_decoder*, int u, char* buf, size_t cap, size_t* need, int* count);
dsr_status dsr_decoder_path_ids(const dsr_decoder*, int u, int which, uint32_t* ids, int cap, int* n);
dsr_status dsr_decoder_final_states_n(const dsr_decoder*, int u, int* n);
dsr_status dsr_decoder_trace_back_succeeded(const dsr_decoder*, int u, int* ok);
typedef struct {
  double  score;        /* decode() return value: double(ac)+double(lm) of the best token */
  float   ac, lm;
  int32_t frames;       /* _frameX after decode (= T-1) */
  int32_t reachedFinal; /* traceBackSucceeded() */
  int32_t nArcs;        /* arcs on the best path incl. epsilon arcs */
  int32_t nWords;       /* output symbols != 0 */
  int32_t status;       /* per-utterance dsr_status (capacity overflow => DSR_E_ALLOCATION) */
  int32_t maxActiveSeen;
  int64_t activeHypos;  /* sum over frames of |_next| (decoder.h:413) */
  int64_t placements;   /* calls of _placeOnList over the utterance (expanded arcs incl. the end expansion) */
  int64_t registerFrames; /* diagnostics: frames that ran on the decoder kernel's register path (rest: memory path) */
  int32_t finalStatesN; /* finalStatesN() (decoder.h:598-608): tokens of _next in a final state after _expandToEnd */
  int32_t laidOutFrames_; /* diagnostics, no part of the result: register-path frames whose placement slots the frame before had laid out
                           * (the other register-path frames built the layout themselves, in the kernel's phases P1 and P2) */
} dsr_decode_result;
/* Batched decode.  score_dev [U][Tmax][nDist] fp32 costs (row t = Distrib::score(t)), nframes_dev [U].
 * Host outputs: res[U]; arcs_out [U][maxPath] (export arc ids, first..last), words_out [U][maxPath]
 * (bestHypo output ids).  arcs_out/words_out may be NULL.
 * Scheduling (results do not depend on it): a batch of more utterances than the device has compute units is decoded in segments of 125 frames, all
 * utterances advancing together, so that they end together (DSR_VITERBI_SEG=<frames> changes the segment, 0 decodes every utterance in one go);
 * a capacity that runs out is per utterance either way (DSR_E_ALLOCATION in its status) -- cfg.arenaTokens then bounds the batch's POOL of
 * back-pointer records, U/8 x (arenaTokens or 8192 x (Tmax+2)) at least, instead of one utterance's. */
dsr_status dsr_decoder_decode_batch(dsr_decoder*, const float* score_dev, const int32_t* nframes_dev, int U,
                                    int Tmax, int nDist, dsr_decode_result* res, int32_t* arcs_out,
                                    uint32_t* words_out, int maxPath, void* stream);
/* The same in two halves: launch enqueues the decode (and the copy of its results to pinned staging memory) on
 * `stream` and returns; collect waits for it and fills the host outputs.  One launch in flight per decoder object. */
dsr_status dsr_decoder_decode_launch(dsr_decoder*, const float* score_dev, const int32_t* nframes_dev, int U,
                                     int Tmax, int nDist, int maxPath, int want_paths, void* stream);
dsr_status dsr_decoder_decode_collect(dsr_decoder*, dsr_decode_result* res, int32_t* arcs_out, uint32_t* words_out);
/* Lattice generation: _Decoder::lattice(), _majorTrace, _minorTrace, _findLNode (asr/decoder/decoder.h:805-953) over the 'worse' chains of
 * _placeOnList (:531-541), for utterance u of the last decode of a decoder created with cfg.latticeTokens > 0 (DSR_E_CONSISTENCY otherwise: the
 * reference's "Must enable lattice generation during decoding.").  eosX: output-lexicon index of eosSymbol (decoder.h:740-745), used when no token
 * reached a final state (:843-851).  Nodes are numbered as the reference numbers them (0 = the initial node, then creation order); edges come in
 * creation order: from, to, input, output, first and last frame, acoustic score and LM score with the penalties and the LM scale taken out
 * (:921-923).  The lattice object is host memory, independent of the decoder afterwards. */
typedef struct dsr_lattice dsr_lattice;
dsr_status dsr_decoder_lattice(dsr_decoder*, int u, uint32_t eosX, dsr_lattice** out);
/* _Decoder::writeGMM(conv, channel, spk, utt, cfrom, score, fileName, frameInterval) (asr/decoder/decoder.h:1018-1102, decoder.i:177-178): the 1-best
 * path of utterance u as runs of equal input symbols -- "# utt cfrom score", then "conv channel start duration label score" per run, the
 * end-of-sentence label skipped; the score column as the shipped code computes it.  Needs lattice bookkeeping (latticeTokens > 0) and the
 * symbols of dsr_decoder_set_symbols; fileName NULL or "": stdout, otherwise the file is appended to.  (writeCTM is not supported by the
 * reference's decoder template either, decoder.h:399-401.) */
dsr_status dsr_decoder_write_gmm(dsr_decoder*, int u, const char* conv, const char* channel, const char* spk, const char* utt, double cfrom, double score,
                                 const char* fileName, double frameInterval);
void       dsr_lattice_destroy(dsr_lattice*);
int        dsr_lattice_num_nodes(const dsr_lattice*);
int        dsr_lattice_num_edges(const dsr_lattice*);
int        dsr_lattice_final_states_n(const dsr_lattice*);      /* finalStatesN() (decoder.h:598-608) */
dsr_status dsr_lattice_get(const dsr_lattice*, int32_t* nodeFinal, int32_t* from, int32_t* to, uint32_t* in, uint32_t* out, int32_t* start,
                           int32_t* end, double* ac, double* lm);   /* any pointer may be NULL */
/* Lattice::write(fileName, useSymbols = false, writeData) (asr/lattice/lattice.cc:715-757); a cyclic lattice is DSR_E_CONSISTENCY (:862-864).
 * Links print under the nodes' current indices (prune/purge renumber them) with their cost when it is not zero (fsm.cc:1171-1178); the data line
 * is "start end ac lm gamma" (lattice.h:151-154).  fileName "" = stdout. */
dsr_status dsr_lattice_write(dsr_lattice*, const char* fileName, int writeData);
/* The operations of asr/lattice's Lattice (lattice.i:79-123) on a lattice object -- the decoder's, an unpacked one or one read from a file.  Host
 * work, as in the reference (a lattice is hundreds to thousands of links).  The object keeps what the reference's keeps between calls: rescoring
 * tokens, probabilities, posteriors, the cached topological order, and _acScale/_lmScale/penalties of the last call.
 *   read          WFST<..>::read(fileName, noSelfLoops, readData) (asr/fsm/fsm.h:3787-3873): the first state named is the initial node; symbols that
 *                 are not numbers are looked up in the lexica (either may be NULL: DSR_E_KEY then)
 *   rescore       Lattice::rescore(lmScale, lmPenalty, silPenalty, silSymbol) (lattice.cc:122-171): best-token pass in topological order with the
 *                 acoustic scale of the last gammaProbs (1.0 before); silenceX = inputLexicon()->index(silSymbol), resolved by the caller
 *   best_hypo     Lattice::bestHypo(useInputSymbols) (:281-306) as symbol indices, first symbol first (the reference joins them with " ")
 *   gamma_probs   Lattice::gammaProbs(acScale, lmScale, lmPenalty, silPenalty, silSymbol) (:309-379): forward/backward over the sorted nodes,
 *                 posterior (as a negative log) per link; returns the lattice's forward probability; the reference's consistency errors
 *                 (forward != backward, negative posterior, a term above LogZero) come back as DSR_E_CONSISTENCY
 *   prune         Lattice::prune(threshold) (:648-693): links with gamma > threshold leave the initial and intermediate nodes, unreachable
 *                 nodes are dropped and the rest renumbered in topological order
 *   prune_edges   Lattice::pruneEdges(edgesN) (:695-713): threshold = the edgesN-th smallest gamma over the links EdgeIterator sees
 *   purge         Lattice::purge() (:776-841): nodes from which no final node can be reached are dropped (links into them stay, as in the reference)
 *   get_state     per link: gamma, still on its node's list; per node: current index, still held by the lattice, forward and backward probability */
dsr_status dsr_lattice_read(const char* fileName, int noSelfLoops, int readData, dsr_lexicon* inputLex, dsr_lexicon* outputLex, dsr_lattice** out);
dsr_status dsr_lattice_rescore(dsr_lattice*, double lmScale, double lmPenalty, double silPenalty, unsigned silenceX, float* score);
dsr_status dsr_lattice_best_hypo(const dsr_lattice*, int useInputSymbols, uint32_t* symbols, int cap, int* n);     /* symbols NULL: length only */
dsr_status dsr_lattice_gamma_probs(dsr_lattice*, double acScale, double lmScale, double lmPenalty, double silPenalty, unsigned silenceX, double* logProb);
dsr_status dsr_lattice_prune(dsr_lattice*, double threshold);
dsr_status dsr_lattice_prune_edges(dsr_lattice*, unsigned edgesN);
dsr_status dsr_lattice_purge(dsr_lattice*);
dsr_status dsr_lattice_get_state(dsr_lattice*, double* gamma, int32_t* edgeLive, int32_t* nodeIndex, int32_t* nodeLive, double* forwardProb,
                                 double* backwardProb);              /* any pointer may be NULL */
/* 1-best writers over the rescoring tokens (call rescore first; DSR_E_CONSISTENCY when no final node holds a token -- the reference dereferences a
 * null token there).  fileName NULL or "": stdout, otherwise appended to.  Rows whose symbol equals endMarker are skipped.
 *   write_ctm        Lattice::writeCTM (lattice.cc:420-477): ";; utt cfrom score", "conv channel start duration word score" per output symbol
 *   write_phone_ctm  Lattice::writePhoneCTM (:479-537): the same per link, input symbols
 *   write_hypo_htk   Lattice::writeHypoHTK (:539-601): "utt.rec", a line per word (flag bit 0: times in 100 ns, bit 1: score), "."
 *   write_word_confs Lattice::writeWordConfs (:603-646): "uttId { {word} conf} ..." with conf = exp(-gamma) of the word's link */
dsr_status dsr_lattice_write_ctm(const dsr_lattice*, const dsr_lexicon* outputLex, const char* conv, const char* channel, const char* spk, const char* utt,
                                 double cfrom, double score, const char* fileName, double frameInterval, const char* endMarker);
dsr_status dsr_lattice_write_phone_ctm(const dsr_lattice*, const dsr_lexicon* inputLex, const char* conv, const char* channel, const char* spk,
                                       const char* utt, double cfrom, double score, const char* fileName, double frameInterval, const char* endMarker);
dsr_status dsr_lattice_write_hypo_htk(const dsr_lattice*, const dsr_lexicon* outputLex, const char* conv, const char* channel, const char* spk,
                                      const char* utt, double cfrom, double score, const char* fileName, int flag, double frameInterval,
                                      const char* endMarker);
dsr_status dsr_lattice_write_word_confs(const dsr_lattice*, const dsr_lexicon* outputLex, const char* fileName, const char* uttId, const char* endMarker);
/* flat image of a lattice for the gather across ranks (north star: "gather decoded lattices/1-best") */
size_t     dsr_lattice_pack_size(const dsr_lattice*);
dsr_status dsr_lattice_pack(const dsr_lattice*, void* buf, size_t bufBytes);
dsr_status dsr_lattice_unpack(const void* buf, size_t bytes, dsr_lattice** out);

/* debug/parity: per-frame token list (list order) of utterance 0 of the last decode with
   cfg.streams == 1 and dumpFrames enabled through dsr_decoder_enable_dump(). */
dsr_status dsr_decoder_enable_dump(dsr_decoder*, int enable);
dsr_status dsr_decoder_get_dump(dsr_decoder*, int64_t* nFrames, const int64_t** frameOff, const int32_t** node,
                                const float** ac, const float** lm, const int32_t** arc);

/* =====================================================================================
 * 6. Whole pipe: 8-ch analysis -> MVDR -> synthesis -> MFCC -> GMM -> Viterbi
 *    (the call sequence of SURVEY.md Appendix C.2-C.4 for a batch of utterances)
 * ===================================================================================== */
typedef struct dsr_pipe dsr_pipe;
dsr_status dsr_pipe_create(const dsr_fb* analysis, const dsr_fb* synthesis, dsr_bf* bf, dsr_mfcc* mfcc,
                           dsr_gmm* gmm, dsr_decoder* dec, int gmmMode, dsr_pipe** out);
void       dsr_pipe_destroy(dsr_pipe*);
/* x_dev [U][C][sampStride]; results as dsr_decoder_decode_batch.  Intermediates live in a workspace
   the pipe grows on demand (never inside a timed region after the first call of a given shape). */
dsr_status dsr_pipe_run(dsr_pipe*, const float* x_dev, const int32_t* nsamp_dev, const int32_t* nsamp_host,
                        int U, int C, int64_t sampStride, dsr_decode_result* res, int32_t* arcs_out,
                        uint32_t* words_out, int maxPath, void* stream);
/* The same in two halves (one batch in flight per pipe object): two pipes on two streams overlap the ragged end of
 * one batch's decode -- utterances finish at different times -- with the front end of the next batch. */
dsr_status dsr_pipe_submit(dsr_pipe*, const float* x_dev, const int32_t* nsamp_dev, const int32_t* nsamp_host,
                           int U, int C, int64_t sampStride, int maxPath, int want_paths, void* stream);
dsr_status dsr_pipe_collect(dsr_pipe*, dsr_decode_result* res, int32_t* arcs_out, uint32_t* words_out);
/* fused = 1: analysis bank and beamformer run as one kernel when dsr_fb_analysis_beamform_supported() -- the channel snapshots are then never
 * written (intermediate 0 is not available, stage time 1 is zero and stage time 0 covers both); default 0 */
dsr_status dsr_pipe_set_fused(dsr_pipe*, int fused);
/* per-stage device time of the last run in milliseconds: [analysis, beamform, synthesis, mfcc, gmm, viterbi] */
dsr_status dsr_pipe_stage_ms(const dsr_pipe*, float ms[6]);
/* device pointers to the intermediates of the last run (borrowed): 0 X, 1 Y, 2 y, 3 feat, 4 scores */
dsr_status dsr_pipe_intermediate(const dsr_pipe*, int which, void** dev, int64_t* bytes);

/* PerfectReconstructionFFTAnalysisBank / PerfectReconstructionFFTSynthesisBank (btk/modulated/modulated.cc:686-970):
 * the 2M-band cosine-modulated pair; prototype of length 2M*m (analysis and synthesis objects each take their own).
 * analysis: x_dev [U][C][sampStride] -> X_dev [U][C][Tmax][2M] complex64, frames(nsamp) = ceil(nsamp/D) + 2m - 1;
 * synthesis: Y_dev [U][Tmax][2M] complex64, nframes_dev [U] -> y_dev [U][outStride] fp32, (nframes - (2m-1)) * D samples. */
typedef struct dsr_prfb dsr_prfb;
dsr_status dsr_prfb_create(const double* prototype, int M, int m, int r, dsr_prfb** out);
void       dsr_prfb_destroy(dsr_prfb*);
int        dsr_prfb_fft_len(const dsr_prfb*);
int        dsr_prfb_block_len(const dsr_prfb*);
int        dsr_prfb_analysis_frames(const dsr_prfb*, int nsamp);
int        dsr_prfb_synthesis_blocks(const dsr_prfb*, int nframes);
dsr_status dsr_prfb_analysis(const dsr_prfb*, const float* x_dev, const int32_t* nsamp_dev, int U, int C,
                             int64_t sampStride, int Tmax, float* X_dev, void* stream);
dsr_status dsr_prfb_synthesis(dsr_prfb*, const float* Y_dev, const int32_t* nframes_dev, int U, int Tmax,
                              int64_t outStride, float* y_dev, void* stream);

/* NormalFFTAnalysisBank (btk/modulated/modulated.cc:121-257) with getWindow (:72-97): windowed STFT, all M bins.
 * windowType 0 rectangle, 1 Hamming, 2 Hanning.  x_dev [U][C][sampStride] -> X_dev [U][C][Tmax][M] complex64;
 * frames(nsamp) = ceil(nsamp / D) + 1 (one zero-input frame, _processingDelay = 1), D = M >> r. */
typedef struct dsr_stft dsr_stft;
dsr_status dsr_stft_create(int M, int r, int windowType, dsr_stft** out);
void       dsr_stft_destroy(dsr_stft*);
int        dsr_stft_frames(const dsr_stft*, int nsamp);
int        dsr_stft_block_len(const dsr_stft*);
dsr_status dsr_stft_analysis(const dsr_stft*, const float* x_dev, const int32_t* nsamp_dev, int U, int C,
                             int64_t sampStride, int Tmax, float* X_dev, void* stream);

/* =====================================================================================
 * 6a. Zelinski post-filter on the beamformer output  (btk/postfilter/postfilter.cc:8-221,350-493:
 *     calcCSD, TimeAlignment, ZelinskiFilter_f, ZelinskiFilter, ZelinskiPostFilter; halfBandShift == false)
 *     type: 1 = Re(sum of CSDs), 2 = |sum| (the SWIG default), +8 = TYPE_ZELINSKI2 (the caller then passes wq() instead of
 *     arrayManifold() to set_manifold).  The densities start from scratch in every utterance (alpha = 0 for its first two
 *     frames, postfilter.cc:463-466); frames with frameX-1 < minFrames pass unfiltered (:471-473).
 *     X_dev [U][C][Tmax][M/2+1] complex64 (the analysis banks' snapshots), Y_dev [U][Tmax][M/2+1] complex64 (beamformer
 *     output) -> out_dev [U][Tmax][M/2+1]; wp1_dev (optional) [U][Tmax][M/2+1] fp32 = getPostFilterWeights().
 * ===================================================================================== */
typedef struct dsr_zelinski dsr_zelinski;
dsr_status dsr_zelinski_create(int fftLen, int chanN, double alpha, int type, int minFrames, dsr_zelinski** out);
void       dsr_zelinski_destroy(dsr_zelinski*);
dsr_status dsr_zelinski_set_manifold(dsr_zelinski*, int fbinX, const double* vec /* chanN complex128 */);   /* setArrayManifoldVector */
/* McCowanPostFilter (postfilter.cc:502-945): same handle type and apply; noise coherence per bin as in SubbandMVDR's setters */
dsr_status dsr_mccowan_create(int fftLen, int chanN, double alpha, int type, int minFrames, float threshold, dsr_zelinski** out);
dsr_status dsr_mccowan_set_noise_matrix(dsr_zelinski*, int fbinX, const double* Rnn /* [C][C] complex128 */);
dsr_status dsr_mccowan_set_diffuse_noise_model(dsr_zelinski*, const double* micPos /* [C][3] */, double sampleRate, double sspeed);
dsr_status dsr_mccowan_diagonal_loading(dsr_zelinski*, int fbinX /* < 0: all bins */, float diagonalWeight);
dsr_status dsr_mccowan_divide_nondiagonal(dsr_zelinski*, float myu);
/* LefkimmiatisPostFilter(output, fftLen, minSV, fbinX1, alpha, type, minFrames, threshold) (postfilter.h:180-202, postfilter.cc:948-1210):
 * the McCowan handle and setters; the pseudo-inverse of every bin's coherence matrix (singular values < minSV dropped) and
 * d^H pinv(R) d are computed inside apply when the matrices or the manifold have changed */
dsr_status dsr_lefkimmiatis_create(int fftLen, int chanN, double minSV, int fbinX1, double alpha, int type, int minFrames, float threshold, dsr_zelinski** out);
dsr_status dsr_zelinski_apply(dsr_zelinski*, const float* X_dev, const float* Y_dev, const int32_t* nframes_dev, int U, int Tmax,
                              float* out_dev, float* wp1_dev, void* stream);
/* The post-filter behind its beamformer: out = postfilter(X, bf(X)) -- ZelinskiPostFilter::setBeamformer (btk/postfilter/postfilter.h:100, postfilter.cc:376-384:
 * the filter takes snapshots and array manifold from the beamformer whose output it filters).  Where the filter streams the snapshots anyway (Zelinski on arrays
 * of other than 2/3/4/6/8 channels) the beamformer's sum is formed in the same pass over them; elsewhere the call is dsr_bf_apply_frames followed by
 * dsr_zelinski_apply.  Y_dev (optional, [U][Tmax][fftLen/2+1] complex64) receives bf(X). */
dsr_status dsr_zelinski_apply_bf(dsr_zelinski*, dsr_bf*, const float* X_dev, const int32_t* nframes_dev, int U, int Tmax,
                                 float* out_dev, float* wp1_dev, float* Y_dev, void* stream);
/* Which kernels dsr_zelinski_apply (bf null) / dsr_zelinski_apply_bf (the beamformer the filter sits behind) launch for a filter of that kind
 * (0 Zelinski, 1 McCowan, 2 Lefkimmiatis) and channel count: path[0] = the cell, path[1] = the kernel's template argument (the channel count of
 * the register kernels, 0 for k_mccowan<0>, the kind for k_pf_wave, 0 for the sum kernels).  The launches take their decisions from the same helper.
 * The switches DSR_PF_SUM (Zelinski: the sum kernels at any size), DSR_PF_NOFUSE (no beamformer sum in the filter's pass), DSR_PF_WAVE (the
 * wave-per-bin kernel at any size) and DSR_PF_MEMSTATE (McCowan / Lefkimmiatis: densities in memory), set to anything, are read on every call.
 * Needs no device. */
enum { DSR_PF_ZEL_REG = 0,             /* k_zelinski_reg<C>: Zelinski, chanN 2, 3, 4, 6, 8 */
       DSR_PF_ZEL_SUM = 1,             /* k_zel_pairs<false> + k_zel_recur: Zelinski at every other size */
       DSR_PF_ZEL_SUM_BF = 2,          /* k_zel_pairs<true> + k_zel_recur: the same behind a beamformer of fixed weights, its sum formed in the same pass */
       DSR_PF_MCCOWAN_REG = 3,         /* k_mccowan<C>: McCowan / Lefkimmiatis, chanN 2, 3, 4, 6, 8 */
       DSR_PF_MCCOWAN_MEM = 4,         /* k_mccowan<0>: the same for any other chanN <= 16 */
       DSR_PF_WAVE = 5 };              /* k_pf_wave<kind>: chanN > 16 (Zelinski only on request: above 16 channels it takes the sum kernels) */
dsr_status dsr_zelinski_path(int kind, int chanN, const dsr_bf* bf, int path[2]);
/* Carried densities for block-wise processing of long streams (BASELINE configs[4]).  The reference operator's auto/cross spectral densities
 * (postfilter.cc:428-497) live as long as the object: carry = 1 makes every apply of the same U continue the recursions where the previous call
 * stopped (stream u of one call = stream u of the next; the start-up alpha = 0 and minFrames count from a stream's own first frame);
 * reset_state begins new streams.  carry = 0 (default): every call is a batch of whole utterances.  chanN <= 64. */
dsr_status dsr_zelinski_carry(dsr_zelinski*, int on);
dsr_status dsr_zelinski_reset_state(dsr_zelinski*);

/* =====================================================================================
 * 6a-2. Single-channel noise suppression: averagePSDEstimator, SpectralSubtractor, WienerFilter
 *     (btk/postfilter/spectralsubtraction.h:20-166, spectralsubtraction.cc:6-347, postfilter.i:150-223).  "6b" was taken by the LPC section.
 * Snapshots X_dev [U][C][Tmax][fftLen/2+1] complex64 (C = the channels of setChannel, in order), or one stream [U][Tmax][fftLen/2+1];
 * nframes_dev [U] optional; rows t >= nframes[u] are written as zero and leave the state as it is.  Outputs are outBins = fftLen/2+1 or fftLen
 * bins a row (the latter with the upper half as the reference leaves it), complex64 or, with outIsDouble, complex128.  What the reference
 * objects keep as long as they live is caller-owned device memory (state_bytes / state_init), so blocks of a long stream chain exactly and one
 * handle serves several states.  Arithmetic is fp64.  Kept quirks and refusals: DESIGN 4.4k.
 * ===================================================================================== */
/* PSDEstimator::writeEstimates / readEstimates (spectralsubtraction.cc:17-49): text, one "%lf" per line; host side, no GPU */
dsr_status dsr_psd_file_write(const char* fn, const double* est, int n);
dsr_status dsr_psd_file_read(const char* fn, double* est, int n);
typedef struct dsr_specsub dsr_specsub;
/* SpectralSubtractor(fftLen, halfBandShift, ft, flooringV) (spectralsubtraction.cc:141-152): training on, subtraction off */
dsr_status dsr_specsub_create(int fftLen, int halfBandShift, float ft, float flooringV, dsr_specsub** out);
void       dsr_specsub_destroy(dsr_specsub*);
/* setChannel(chan, alpha) (:185-189): one more channel with its own averagePSDEstimator(fftLen/2, alpha); alpha < 0 = average of the stored
   samples at stopTraining, alpha >= 0 = recursive average.  Channels are added before the state is sized. */
dsr_status dsr_specsub_set_channel(dsr_specsub*, double alpha);
int        dsr_specsub_chan_n(const dsr_specsub*);
int        dsr_specsub_fft_len(const dsr_specsub*);
dsr_status dsr_specsub_set_noise_over_estimation_factor(dsr_specsub*, float ft);     /* spectralsubtraction.h:75-77 */
dsr_status dsr_specsub_start_training(dsr_specsub*);                                 /* :83-85 */
/* stopTraining (:87-91): the flag, and average() of every channel with alpha < 0 in the state.  A channel without a stored sample divides zero by
   zero in the reference: here DSR_E_ARITHMETIC, the flag is off and no estimate changes.  Synchronous (it reads the sample counts).
   state_dev NULL: the flag alone. */
dsr_status dsr_specsub_stop_training(dsr_specsub*, void* state_dev, int U, void* stream);
dsr_status dsr_specsub_set_noise_subtraction(dsr_specsub*, int on);                  /* start / stopNoiseSubtraction (:103-109) */
int        dsr_specsub_is_training(const dsr_specsub*);
int        dsr_specsub_is_subtracting(const dsr_specsub*);
size_t     dsr_specsub_state_bytes(const dsr_specsub*, int U);
dsr_status dsr_specsub_state_init(dsr_specsub*, void* state_dev, int U, void* stream);            /* zero estimates, no samples: a new object */
dsr_status dsr_specsub_clear_noise_samples(dsr_specsub*, void* state_dev, int U, void* stream);   /* clearNoiseSamples (:93-96) */
dsr_status dsr_specsub_clear(dsr_specsub*, void* state_dev, int U, void* stream);                 /* clear (:98-101): also forgets the first sample */
/* next() for every frame (spectralsubtraction.cc:198-267): per channel the training sample first, then the subtraction with the current estimate;
   without subtraction the channel average.  out_dev NULL: training only (averagePSDEstimator::addSample, :89-119). */
dsr_status dsr_specsub_apply(dsr_specsub*, const float* X_dev, const int32_t* nframes_dev, int U, int Tmax, void* out_dev, int outBins, int outIsDouble,
                             void* state_dev, void* stream);
/* what 0: getEstimate() [fftLen/2+1]; 1: the sum of the stored samples [fftLen/2+1]; 2: {stored samples, first sample seen} (synchronous) */
dsr_status dsr_specsub_state_read(const dsr_specsub*, const void* state_dev, int U, int what, int u, int chan, double* host_out, size_t outDoubles);
dsr_status dsr_specsub_state_write_estimate(dsr_specsub*, void* state_dev, int U, int u /* < 0: all */, int chan, const double* est);
/* readNoiseFile(fn, idx) (spectralsubtraction.h:111-114): stops training, then loads channel idx's estimate of every utterance; writeNoiseFile of utterance u */
dsr_status dsr_specsub_read_noise_file(dsr_specsub*, const char* fn, int idx, void* state_dev, int U);
dsr_status dsr_specsub_write_noise_file(const dsr_specsub*, const char* fn, int idx, const void* state_dev, int U, int u);

typedef struct dsr_wiener dsr_wiener;
/* WienerFilter(target, noise, halfBandShift, alpha, flooringV, beta) (spectralsubtraction.cc:269-285); noiseLen != fftLen is DSR_E_DIMENSION as
   there; halfBandShift is accepted and, as there, refused by the first apply (DSR_E_ERROR).  beta is held as a float, as there. */
dsr_status dsr_wiener_create(int fftLen, int noiseLen, int halfBandShift, float alpha, float flooringV, double beta, dsr_wiener** out);
void       dsr_wiener_destroy(dsr_wiener*);
dsr_status dsr_wiener_set_noise_amplification_factor(dsr_wiener*, double beta);      /* spectralsubtraction.h:146 */
dsr_status dsr_wiener_set_updating_noise_psd(dsr_wiener*, int on);                   /* start / stopUpdatingNoisePSD (:149-150) */
/* The reference's frame counter and PSD memories live as long as the object (reset() touches the sources only).  carry = 1: every apply goes on
   where the state stands; carry = 0 (default): every call starts each utterance like a new object and leaves its end state behind. */
dsr_status dsr_wiener_carry(dsr_wiener*, int on);
size_t     dsr_wiener_state_bytes(const dsr_wiener*, int U);
dsr_status dsr_wiener_state_init(const dsr_wiener*, void* state_dev, int U, void* stream);
dsr_status dsr_wiener_reset_state(const dsr_wiener*, void* state_dev, int U, void* stream);
/* next() for every frame (spectralsubtraction.cc:293-341): S_dev, N_dev [U][Tmax][fftLen/2+1] complex64 (N_dev may be NULL while updating is off) */
dsr_status dsr_wiener_apply(dsr_wiener*, const float* S_dev, const float* N_dev, const int32_t* nframes_dev, int U, int Tmax, void* out_dev, int outBins,
                            int outIsDouble, void* state_dev, void* stream);
/* what 0: _prevPSDs [fftLen/2+1]; 1: _prevPSDn [fftLen/2+1]; 2: frames seen [1] */
dsr_status dsr_wiener_state_read(const dsr_wiener*, const void* state_dev, int U, int what, int u, double* host_out, size_t outDoubles);

/* =====================================================================================
 * 6a-3. Two-channel binary masks and their threshold estimators: BinaryMaskFilter, KimBinaryMaskFilter, IIDBinaryMaskFilter,
 *     KimITDThresholdEstimator, IIDThresholdEstimator, FDIIDThresholdEstimator
 *     (btk/postfilter/binauralprocessing.h, binauralprocessing.cc:12-928, postfilter.i:254-440)
 * L_dev, R_dev [U][Tmax][fftLen/2+1] complex64.  The masks keep the smoothed mask of the last frame (float [U][fftLen/2+1], initially 1) in
 * caller-owned memory, with carry as in dsr_wiener_carry.  The estimators add to caller-owned fp64 accumulators that run from block to block
 * until reset_state; the host-side finaliser turns one utterance's accumulators into the threshold.  Kept quirks and refusals: DESIGN 4.4k.
 * ===================================================================================== */
typedef struct dsr_binmask dsr_binmask;
#define DSR_MASK_BASE 0   /* BinaryMaskFilter: next() only advances, the output stays zero (binauralprocessing.cc:94-98) */
#define DSR_MASK_KIM  1   /* KimBinaryMaskFilter (:121-176); dPowerCoeff is stored and unused */
#define DSR_MASK_IID  2   /* IIDBinaryMaskFilter (:431-485) */
dsr_status dsr_binmask_create(int kind, unsigned chanX, int fftLen, float threshold, float alpha, float dEta, float dPowerCoeff, dsr_binmask** out);
void       dsr_binmask_destroy(dsr_binmask*);
dsr_status dsr_binmask_set_threshold(dsr_binmask*, float threshold);                 /* binauralprocessing.h:53 */
double     dsr_binmask_threshold(const dsr_binmask*);                                /* :55 */
/* setThresholds (:79-92): the first call only allocates (zeros here, uninitialised there), later calls copy bins 1..fftLen/2.  Once they exist,
   IIDBinaryMaskFilter uses them, rounded to float, in place of the scalar, which then holds the last bin's value after an apply. */
dsr_status dsr_binmask_set_thresholds(dsr_binmask*, const double* thresholds, int n);
dsr_status dsr_binmask_thresholds(const dsr_binmask*, double* out, int n, int32_t* exists);     /* getThresholds; *exists = 0 while NULL there */
dsr_status dsr_binmask_carry(dsr_binmask*, int on);
size_t     dsr_binmask_state_bytes(const dsr_binmask*, int U);
dsr_status dsr_binmask_state_init(const dsr_binmask*, void* state_dev, int U, void* stream);
dsr_status dsr_binmask_reset_state(const dsr_binmask*, void* state_dev, int U, void* stream);
/* masking1 for every frame.  mu_dev (optional) float [U][Tmax][fftLen/2+1] the smoothed mask, itd_dev (optional) double, same shape, Kim's ITD */
dsr_status dsr_binmask_apply(dsr_binmask*, const float* L_dev, const float* R_dev, const int32_t* nframes_dev, int U, int Tmax, void* out_dev, int outBins,
                             int outIsDouble, float* mu_dev, double* itd_dev, void* state_dev, void* stream);
dsr_status dsr_binmask_state_read(const dsr_binmask*, const void* state_dev, int U, int u, float* host_out, size_t outFloats);

typedef struct dsr_thest dsr_thest;
#define DSR_THEST_KIM   0
#define DSR_THEST_IID   1
#define DSR_THEST_FDIID 2
/* The constructors (binauralprocessing.cc:232-287, :525-538, :702-763).  minThreshold == maxThreshold selects the built-in range.  The candidate
   table is the reference's float loop; a loop that yields more values than the (int)((max-min)/width + 1.5) its arrays hold writes past them
   there: DSR_E_INDEX here.  A width that does not advance the threshold is DSR_E_PARAMETER, as is sampleRate 0 with a band.  More than 1024 candidates are DSR_E_DIMENSION.  A band beyond fftLen/2+1 bins is DSR_E_DIMENSION
   (the snapshots hold no more).  FDIID ignores minFreq, maxFreq, sampleRate.  No GPU needed. */
dsr_status dsr_thest_create(int kind, int fftLen, float minThreshold, float maxThreshold, float width, float minFreq, float maxFreq, int sampleRate, float dEta,
                            float dPowerCoeff, dsr_thest** out);
void       dsr_thest_destroy(dsr_thest*);
int        dsr_thest_kind(const dsr_thest*);
int        dsr_thest_n_cand(const dsr_thest*);          /* the arrays' length */
int        dsr_thest_n_loop(const dsr_thest*);          /* the candidates the loop reaches (<= n_cand) */
dsr_status dsr_thest_candidates(const dsr_thest*, float* out, int n);
dsr_status dsr_thest_bin_range(const dsr_thest*, int32_t* out2);
/* per utterance: Kim cost, mean_T, mean_I, sigma_T, sigma_I [nCand] each; IID mean_T, mean_I, sigma_T, sigma_I, Y4_T, Y4_I [nCand] each;
   FDIID Y4, mean, sigma [fftLen/2+1][nCand] each; then the sample count */
size_t     dsr_thest_acc_doubles(const dsr_thest*);
size_t     dsr_thest_state_bytes(const dsr_thest*, int U);
dsr_status dsr_thest_state_init(const dsr_thest*, void* state_dev, int U, void* stream);
dsr_status dsr_thest_reset_state(const dsr_thest*, void* state_dev, int U, void* stream);       /* reset() (:409-426, :664-683, :906-928) */
/* accumStats1 for every frame (:314-353, :549-605, :800-844), added to the accumulators */
dsr_status dsr_thest_run(dsr_thest*, const float* L_dev, const float* R_dev, const int32_t* nframes_dev, int U, int Tmax, void* state_dev, void* stream);
dsr_status dsr_thest_state_read(const dsr_thest*, const void* state_dev, int U, int u, double* host_out, size_t outDoubles);
/* calcThreshold (:382-407, :634-662, :873-904) on the host from one utterance's accumulators; inPlace != 0 divides acc as the reference does (a second
   call then differs, as there).  cost (optional): getCostFunction, [nCand], FDIID [fftLen/2+1][nCand]; thresholds (optional, FDIID): getThresholds */
dsr_status dsr_thest_calc_threshold(const dsr_thest*, double* acc, size_t accDoubles, int inPlace, double* threshold, int32_t* index, double* cost,
                                    size_t costDoubles, double* thresholds, int thresholdsN);

/* SubbandMMI (btk/beamformer/beamformer.h:264-312, beamformer.cc:1753-2319; beamformer.i:255-287): one generalized sidelobe canceller per
 * sound source; the output is the target source's GSC output, Zelinski post-filtered (pfType: postfilter.h:63-69 bits -- 0x01 real part /
 * 0x02 magnitude of the summed cross densities, 0x08 steer with the beamformer's own vector; 0 = no post-filter) and, after
 * use_binary_mask, zeroed (avgFactor < 0) or replaced by avgFactor x the recursive average of earlier outputs where another source's output
 * is stronger (type 0: the other sources' GSC outputs, 1: every source's upper-branch output).
 *   calc_weights      = calcWeights(sampleRate, delays[nSource][chanN])            one linear constraint per source (:1769-1780)
 *   calc_weights_n    = calcWeightsN(sampleRate, delays, NC)                       NC constraints: target + NC-1 nulls (:1788-1811)
 *   set_active_weights_f    = setActiveWeights_f(fbinX, packedWeights[rows][cols], option)      rows = nSource, cols = 2 (chanN - NC); option 1
 *                             resolves the scaling of the demixing matrix through its pseudo-inverse (:1821-1880)
 *   set_hi_active_weights_f = setHiActiveWeights_f(fbinX, pkdWa, pkdwb, option)    (:1891-1968)
 *   get: kind 0 wq [M][C], 1 wl [M][C], 2 B [M][C][C-NC], 3 array manifold [M][C], 4 wa [M][C-NC] of one source, complex128
 *   apply = next() for a batch: X_dev [U][chanN][Tmax][bins] complex64 snapshots -> Y_dev [U][Tmax][out_bins], bins = dsr_mmi_bins()
 *           (fftLen/2+1, or fftLen with halfBandShift); every utterance starts like a fresh object (frame counter, densities, average).
 *   pfType bit 0x04 = TYPE_APAB (beamformer.cc:2047-2049,2177-2179; ApabFilter postfilter.cc:225-340, channelX = chanN/2; it takes precedence
 *           over the Zelinski bits): the filter touches the bins below fftLen/2 only, so without halfBandShift the output frame is not
 *           conjugate-symmetric and ALL fftLen bins are handed over: out_bins = dsr_mmi_out_bins() = fftLen then (bins above fftLen/2 as the
 *           reference leaves them: conj of the unfiltered lower bin, or the mask's value); otherwise out_bins = bins.
 * Errors as the reference raises them: DSR_E_ERROR "call calcWeightsX() once" / wrong number of rows, DSR_E_DIMENSION for packed sizes and
 * bins. */
typedef struct dsr_mmi dsr_mmi;
dsr_status dsr_mmi_create(int fftLen, int chanN, int halfBandShift, int targetSourceX, int nSource, int pfType, double alpha, dsr_mmi** out);
void       dsr_mmi_destroy(dsr_mmi*);
int        dsr_mmi_bins(const dsr_mmi*);
int        dsr_mmi_out_bins(const dsr_mmi*);
int        dsr_mmi_chan_n(const dsr_mmi*);
int        dsr_mmi_fft_len(const dsr_mmi*);
dsr_status dsr_mmi_use_binary_mask(dsr_mmi*, double avgFactor, unsigned fwidth, unsigned type);
dsr_status dsr_mmi_calc_weights(dsr_mmi*, double sampleRate, const double* delays /*[nSource][chanN]*/);
dsr_status dsr_mmi_calc_weights_n(dsr_mmi*, double sampleRate, const double* delays /*[nSource][chanN]*/, unsigned NC);
dsr_status dsr_mmi_set_active_weights_f(dsr_mmi*, unsigned fbinX, const double* packedWeights, size_t rows, size_t cols, int option);
dsr_status dsr_mmi_set_hi_active_weights_f(dsr_mmi*, unsigned fbinX, const double* pkdWa, size_t nWa, const double* pkdwb, size_t nWb, int option);
dsr_status dsr_mmi_get(const dsr_mmi*, int srcX, int kind, double* out, size_t outDoubles);
dsr_status dsr_mmi_apply(dsr_mmi*, const float* X_dev, const int32_t* nframes_dev, int U, int Tmax, float* Y_dev, void* stream);

/* Single-channel WPE dereverberation of a subband sequence (SingleChannelWPEDereverberationFeature, btk/dereverberation/
 * dereverberation.cc:28-300; SWIG defaults iterationsN 2, loadDb -20, bandWidth 0, sampleRate 16000).  Y_dev [U][Nmax][M/2+1]
 * complex64 -> out_dev same shape; gn_dev (optional) [U][M/2+1][upperN-lowerN+1] complex128 = the prediction filters.  The
 * filters start from zero for every utterance (nextSpeaker() semantics). */
dsr_status dsr_wpe_single(const float* Y_dev, const int32_t* nframes_dev, int U, int Nmax, int fftLen, int lowerN, int upperN,
                          int iterationsN, double loadDb, double bandWidth, double sampleRate, float* out_dev, double* gn_dev, void* stream);
/* the next utterance -- or the next block of a long stream -- of an object that was reset() but not nextSpeaker()-ed (dereverberation.cc:258-277:
 * reset() keeps _gn): gn_dev (required) holds the filters the call before left; they seed the first theta_n and are replaced by this call's */
dsr_status dsr_wpe_single_continue(const float* Y_dev, const int32_t* nframes_dev, int U, int Nmax, int fftLen, int lowerN, int upperN,
                                   int iterationsN, double loadDb, double bandWidth, double sampleRate, float* out_dev, double* gn_dev, void* stream);
/* MultiChannelWPEDereverberation (dereverberation.h:89-157, dereverberation.cc:281-586): Y_dev [U][chanN][Nmax][fftLen/2+1] complex64 -> out_dev same shape;
 * gn_dev [U][chanN][fftLen/2+1][chanN*(upperN-lowerN+1)] complex128 (required).  filterChan < 0: own filter per channel; >= 0: all channels through that
 * channel's filter = the reference's getOutput when that channel's feature asks for the frame first (dereverberation.cc:381).  The filters start from zero
 * (nextSpeaker() semantics).  Two paths: while the packed chanN P x chanN P matrix fits the LDS working set (chanN P up to about 133) one workgroup per
 * (utterance, subband, channel) does it all; above that, up to chanN P = 1024 (64 channels x 16 taps), the matrices are built and factorised in a device
 * workspace on the fp64 MFMA; beyond 1024 DSR_E_DIMENSION.  The environment variable DSR_WPE_MULTI_TILED=1 takes the second path at any size. */
dsr_status dsr_wpe_multi(const float* Y_dev, const int32_t* nframes_dev, int U, int chanN, int Nmax, int fftLen, int lowerN, int upperN, int iterationsN,
                         double loadDb, double bandWidth, double sampleRate, int filterChan, float* out_dev, double* gn_dev, void* stream);
/* the next block of a long stream -- or the next utterance -- of an object that was reset() but not nextSpeaker()-ed (dereverberation.cc:341-354, :575-583:
 * reset() keeps _Gn): gn_dev (required) holds the filters the call before left; they seed the first theta_n and are replaced by this call's */
dsr_status dsr_wpe_multi_continue(const float* Y_dev, const int32_t* nframes_dev, int U, int chanN, int Nmax, int fftLen, int lowerN, int upperN,
                                  int iterationsN, double loadDb, double bandWidth, double sampleRate, int filterChan, float* out_dev, double* gn_dev,
                                  void* stream);

/* =====================================================================================
 * 6b. LPC / MVDR spectral envelopes  (btk/feature/lpc.cc:44-207, lpc.h:134-195,291-331:
 *     WarpMVDRFeature, BurgMVDRFeature, WarpLPCFeature, BurgLPCFeature)
 *     method 0 = WarpFeature (warped autocorrelation + Levinson-Durbin), 1 = BurgFeature;
 *     kind 0 = MVDR envelope, 1 = LPC envelope.  frames_dev [T][dim] fp32 (the Hamming-windowed
 *     blocks) -> out_dev [T][dim/2+1] fp64.  order >= dim/2+1 => DSR_E_PARAMETER (lpc.h:126-127).
 *     Below them the header's other two operators: WarpedTwiceMVDRFeature and SpectralSmoothing.
 * ===================================================================================== */
typedef struct dsr_lpc dsr_lpc;
dsr_status dsr_lpc_create(int dim, int order, int correlate, float warp, int method, int kind, dsr_lpc** out);
void       dsr_lpc_destroy(dsr_lpc*);
int        dsr_lpc_size(const dsr_lpc*);
dsr_status dsr_lpc_run(dsr_lpc*, const float* frames_dev, int64_t T, double* out_dev, void* stream);

/* WarpedTwiceMVDRFeature (btk/feature/lpc.h:205-246, lpc.cc:212-468): the warped MVDR envelope whose coefficient sequence is warped a second
 * time, by `_rewarp`, through a chain of dim first-order all-pass stages (trans_longchain, lpc.cc:374-389).  warpFactorFixed: _rewarp follows
 * from warp and sensibility alone (lpc.cc:352-355); otherwise from |R1/R0| of the frame's first `correlate` samples (lpc.cc:392-407,425-428);
 * correlate < 10 means dim (lpc.cc:348).  order >= dim/2+1 => DSR_E_PARAMETER (lpc.cc:349-350); correlate > dim => DSR_E_PARAMETER (R1R0 would
 * read past the frame).  The fp32 part is the reference's operation for operation, double promotions included, with two departures: R holds the
 * order+2 values that autoCorrelation writes (the reference allocates order+1, lpc.cc:214,260), and the weights of PC (lpc.cc:436) are signed
 * as in MVDRFeature (lpc.h:156) where the reference's unsigned expression wraps the negative ones around.
 * run: frames_dev [T][dim] fp32 -> out_dev [T][dim/2+1] fp64.  warp_dev [T] (or NULL: the plan's warp) is each frame's first-stage warp, so
 * that one batch can hold several speakers.  pa_dev [T][dim+1] and rewarp_dev [T] (either may be NULL) receive the re-warped sequence
 * PA[0..dim] before fftPower (lpc.cc:447-448) and the frame's _rewarp. */
typedef struct dsr_wtmvdr dsr_wtmvdr;
dsr_status dsr_wtmvdr_create(int dim, int order, int correlate, float warp, int warpFactorFixed, float sensibility, dsr_wtmvdr** out);
void       dsr_wtmvdr_destroy(dsr_wtmvdr*);
int        dsr_wtmvdr_size(const dsr_wtmvdr*);
dsr_status dsr_wtmvdr_run(dsr_wtmvdr*, const float* frames_dev, const float* warp_dev, int64_t T, double* out_dev, float* pa_dev, float* rewarp_dev,
                          void* stream);
/* measurement (tools/bench_wtmvdr.py): with timing on, dsr_wtmvdr_run brackets its launches with events and waits for them; kernel_ms then gives
 * the last call's milliseconds in the frame transpose, the autocorrelation/Levinson/PC kernel, the all-pass chain and the transform */
dsr_status dsr_wtmvdr_set_timing(dsr_wtmvdr*, int on);
dsr_status dsr_wtmvdr_kernel_ms(const dsr_wtmvdr*, double* ms4);
/* SpectralSmoothing::next (lpc.h:342-358, lpc.cc:485-529): out = mult * adjust_to, mult = max of the 5-tap smoothed adjust_from over the max of
 * adjust_to (100 * the former where the latter is below 0.01).  All three [T][size] fp64; out_dev may be adjust_to_dev.  size < 2 =>
 * DSR_E_PARAMETER (the reference's size()-2 wraps around there, lpc.cc:500,507). */
dsr_status dsr_specsmooth_run(const double* adjust_to_dev, const double* adjust_from_dev, int64_t T, int size, double* out_dev, void* stream);

/* =====================================================================================
 * 6c. The scalar feature operators of btk/feature/feature.{h,cc} (csrc/k_featops.hip): SignalPower, ZeroCrossingRateHamming, YINPitch,
 *     SpikeFilter, SpikeFilter2, ALog, Normalize, Threshold, Amplification, SpectralResampling, SphinxMel
 *
 * Every call takes device arrays [U][Tmax][dim], nframes_dev int32 [U] (NULL: Tmax frames each) and a stream; frames at or past an
 * utterance's count come out zero.  The operation order and the float / double of every intermediate are the reference's, so the results
 * equal a restatement of its lines bit for bit (ALog: up to the device's fp64 log10).
 * ===================================================================================== */
/* SignalPowerFeature::next (feature.cc:1360-1378): y [U][Tmax][1] = float(sum_i double(x[i])^2 / dim / (65536^2 / 4)), i ascending */
dsr_status dsr_signal_power_run(const float* x_dev, const int32_t* nframes_dev, int U, int Tmax, int dim, float* y_dev, void* stream);
/* ZeroCrossingRateHammingFeature::next (feature.cc:3545-3577): y [U][Tmax][1]; the window 0.54 - 0.46 cos(2 pi i / (dim-1)) is built on the
 * host in fp64, the float sum is widened, added to and rounded back at every step over dim-1 terms, then divided by float(dim); x >= 0 counts
 * as positive (-0.0 too) */
dsr_status dsr_zcr_hamming_run(const float* x_dev, const int32_t* nframes_dev, int U, int Tmax, int dim, float* y_dev, void* stream);
/* YINPitchFeature::next (feature.cc:3584-3634): W = dim/2; d(tau) = sum_{j<W} (x[j] - x[j+tau])^2 in fp32, j ascending; tmp2 += d(tau) and
 * y(tau) = d(tau) * float(tau) / tmp2 in fp32, tau = 1..W-1, y(0) = 1; the first tau with y(tau) < threshold and y(tau-1) < y(tau) ends the
 * search with lag tau-1.  pitch_dev [U][Tmax][1] = float(double(samplerate) / double(lag)), 0 without a hit or with lag 0 (a silent frame's
 * 0/0 fails both comparisons).  value_dev (may be NULL) [U][Tmax] = y at the tau that ended the search, y(W-1) when none did; chunks_dev
 * (may be NULL) [U][Tmax] = the chunks of 64 lags the frame's wavefront evaluated (tools/bench_featops.py).  dim < 2 => DSR_E_DIMENSION.
 * dsr_yin_kernel(dim): the kernel a frame length selects -- 4 or 1 frames a workgroup with the frame in LDS, 0 the frame read from global
 * memory. */
dsr_status dsr_yin_pitch_run(const float* x_dev, const int32_t* nframes_dev, int U, int Tmax, int dim, unsigned samplerate, float threshold, float* pitch_dev,
                             float* value_dev, int32_t* chunks_dev, void* stream);
int        dsr_yin_kernel(int dim);
/* SpikeFilter::next (feature.cc:3639-3696), q = (tapN-1)/2: y[i] = x[i] for i < q, the median of x[i-q..i+q] for q <= i < dim-2q; y[dim-2q..dim-1]
 * stays zero as in the reference, which never writes it.  tapN < 3, dim < tapN (the reference's refusals) and an even tapN (its window would
 * read x[dim]) => DSR_E_DIMENSION; check: the same refusals without a device. */
dsr_status dsr_spike_filter_check(int dim, int tapN);
dsr_status dsr_spike_filter_run(const float* x_dev, const int32_t* nframes_dev, int U, int Tmax, int dim, int tapN, float* y_dev, void* stream);
/* SpikeFilter2::next (feature.cc:3701-3776): the serial spike detector, frames in order, utterances in parallel.  meanslope_dev float [U] and
 * count_dev int32 [U] are the reference's _meanslope and _count: set them to startslope and 0 for reset(); the call continues from them and
 * leaves them behind, so an utterance run as consecutive calls equals one call.  A block is staged in LDS: dim > 16000 => DSR_E_DIMENSION. */
dsr_status dsr_spike_filter2_run(const float* x_dev, const int32_t* nframes_dev, int U, int Tmax, int dim, unsigned width, float maxslope, float thresh, float alpha,
                                 float* meanslope_dev, int32_t* count_dev, float* y_dev, void* stream);
/* ALogFeature / NormalizeFeature (feature.cc:1383-1514).  state_dev double [U][2] = (min, max) of the source as the operator holds them;
 * state_init sets (HUGE, -HUGE), i.e. nextSpeaker().  runon = 0: reset() semantics, the pair is taken over the whole utterance (all dim
 * elements of every frame) from (HUGE, -HUGE) and every frame is processed with it -- frame t of the output from frame t of the input, what the
 * reference computes over a random-access source.  runon = 1: the pair continues from state_dev and frame t sees frames 0..t.  Either way the
 * final pair is left in state_dev (NULL: scratch that starts fresh).
 * alog: y [U][Tmax][1] = float(m * log10(val)), val = double(float(max / 10^a) + x[t][0]), 1 where val <= 0 (the sum is a float sum, as the
 * reference's expression types it).  normalize: y [U][Tmax][dim] = float(x * factor + add), factor = (ymax - ymin) / (max - min),
 * add = ymin - min * factor in fp64; a zero range divides by zero as IEEE does. */
dsr_status dsr_minmax_state_init(double* state_dev, int U, void* stream);
dsr_status dsr_alog_run(const float* x_dev, const int32_t* nframes_dev, int U, int Tmax, int dim, double m, double a, int runon, double* state_dev, float* y_dev,
                        void* stream);
dsr_status dsr_normalize_run(const float* x_dev, const int32_t* nframes_dev, int U, int Tmax, int dim, double ymin, double ymax, int runon, double* state_dev,
                             float* y_dev, void* stream);
/* ThresholdFeature (feature.cc:1519-1560): compare 1 "upper" (v >= thresh -> value), -1 "lower" (v <= thresh -> value), 0 "both" (v >= thresh ->
 * value, v <= -thresh -> -value); threshold_mode maps the name, any other is DSR_E_KEY.  AmplificationFeature (feature.cc:3927-3941):
 * y = float(double(x) * amplify). */
dsr_status dsr_threshold_mode(const char* mode, int* compare);
dsr_status dsr_threshold_run(const float* x_dev, const int32_t* nframes_dev, int U, int Tmax, int dim, double value, double thresh, int compare, float* y_dev,
                             void* stream);
dsr_status dsr_amplify_run(const float* x_dev, const int32_t* nframes_dev, int U, int Tmax, int dim, double amplify, float* y_dev, void* stream);
/* SpectralResamplingFeature (feature.cc:1565-1602): x double [U][Tmax][srcN] -> y double [U][Tmax][outN], outN = len or, for len 0, srcN;
 * r = ratio * float(srcN) / float(outN); y[c] = double(float(wgt * x[low] + (1 - wgt) * x[low+1])) with float exact = c r, low = unsigned(c r),
 * float wgt = (low+1) - exact.  r > 1 => DSR_E_CONSISTENCY.  Where low+1 = srcN the reference reads one element past the end: with weight
 * exactly 0 that term is taken as 0, with any other weight (or low >= srcN) the configuration is DSR_E_DIMENSION.  size: outN and the refusals,
 * without a device. */
dsr_status dsr_spectral_resample_size(int srcN, double ratio, int len, int* outN);
dsr_status dsr_spectral_resample_run(const double* x_dev, const int32_t* nframes_dev, int U, int Tmax, int srcN, double ratio, int len, double* y_dev, void* stream);
/* SphinxMelFeature (feature.cc:2303-2385): the filterN x powerN matrix is built on the host in fp64 exactly as written there (unnormalised
 * triangles, k from 1, the break at the first bin above the right edge; lowerF = upperF = 0 gives an all-zero matrix); upperF above Nyquist is
 * DSR_E_ERROR.  apply: x double [U][Tmax][powerN] -> y double [U][Tmax][filterN], a row times the frame in fp64, k ascending. */
typedef struct dsr_sphinx_mel dsr_sphinx_mel;
dsr_status dsr_sphinx_mel_create(unsigned fftN, unsigned powerN, float sampleRate, float lowerF, float upperF, unsigned filterN, dsr_sphinx_mel** out);
void       dsr_sphinx_mel_destroy(dsr_sphinx_mel*);
int        dsr_sphinx_mel_size(const dsr_sphinx_mel*);
int        dsr_sphinx_mel_power_n(const dsr_sphinx_mel*);
dsr_status dsr_sphinx_mel_filters(const dsr_sphinx_mel*, double* A_host /* [filterN][powerN] */);
dsr_status dsr_sphinx_mel_apply(dsr_sphinx_mel*, const double* x_dev, const int32_t* nframes_dev, int U, int Tmax, double* y_dev, void* stream);

/* =====================================================================================
 * 6d. Sample-rate conversion (csrc/src_kernels.hip, csrc/src.cpp)
 *     stands for SamplerateConversionFeature (btk/feature/feature.h:794-816, feature.cc:1607-1699), which wraps libsamplerate.  libsamplerate is
 *     not reproduced: the converter is defined here, band-limited interpolation with a Kaiser-windowed sinc, and its output bits are its own.
 * Rates are unsigned integers; g = gcd(src, dst), L = dst/g, M = src/g, s = min(1, L/M).  Output n sits at input time n M / L:
 * base = floor(n M / L) in 64-bit integers, phase p = (n M) mod L, frac = p / L.  N input samples give floor(N L / M) outputs; the input is zero
 * before sample 0 and after sample N-1.
 *   "fastest", "medium", "best" (the reference's names, feature.cc:1615-1626): Z = 10, 16, 32 zero crossings, Kaiser beta = 7.0, 9.5, 12.0,
 *   cutoff c = 0.84, 0.90, 0.95; K = ceil(Z / s); y[n] = sum_{j=-K+1..K} h_p[j] x[base + j], h_p[j] = s c sinc(s c d) w(d s / Z), d = frac - j,
 *   sinc(v) = sin(pi v) / (pi v), w(v) = I0(beta sqrt(1 - v^2)) / I0(beta) for |v| < 1, else 0; each phase's 2K taps are divided by their sum (DC
 *   passes exactly).  The table [L][2K] is computed on the host in fp64 at create, rounded to fp32 and uploaded once; the device sums in fp32: two
 *   chains acc = fmaf(h, x, acc) from 0, over every other tap each with j ascending, and their rounded sum -- the same on every path and for every
 *   split of the work.
 *   "zoh": y[n] = x[base] (K = 0).  "linear": y[n] = x[base] + f (x[base+1] - x[base]), f = float(p) / float(L), each operation rounded to
 *   fp32 and none fused (K = 1).
 * create refuses any other name with the reference's "Cannot recognize type (%s) of sample rate converter." (DSR_E_CONSISTENCY), a zero rate
 * and a table 2K L above 2^22 entries (DSR_E_PARAMETER).  Equal rates are a copy, whatever the method (K = 0).
 * ===================================================================================== */
typedef struct dsr_src dsr_src;
enum { DSR_SRC_TABLE_LDS = 0,            /* the coefficient table sits in LDS beside the input tile */
       DSR_SRC_TABLE_MEM = 1,            /* it does not fit (or DSR_SRC_TABLE=mem): read through the cache */
       DSR_SRC_TABLE_UNIFORM = 2,        /* L = 1, integer decimation: one row, read with wave-uniform addresses */
       DSR_SRC_TABLE_NONE = 3 };         /* zoh, linear, equal rates */
enum { DSR_SRC_INPUT_LDS = 0,            /* a workgroup stages the input span of a run of outputs in LDS */
       DSR_SRC_INPUT_DIRECT = 1 };       /* straight from memory: zoh, linear, and ratios whose 2K taps alone exceed a tile */
dsr_status dsr_src_create(unsigned srcRate, unsigned dstRate, const char* method, dsr_src** out);
void       dsr_src_destroy(dsr_src*);
dsr_status dsr_src_ratio(const dsr_src*, int32_t ratio[3] /* L, M, K */);
int64_t    dsr_src_out_samples(const dsr_src*, int64_t nIn);            /* floor(nIn L / M): what a one-shot call, or a flushed stream, gives */
/* the most outputs one call with carried state gives for nIn input samples (outputs held back by earlier blocks included): the least outStride */
int64_t    dsr_src_block_out_bound(const dsr_src*, int64_t nIn);
/* the fp32 table of a sinc method as the definition orders it: table [L][2K], row p = phase p, j = -K+1 .. K (host) */
dsr_status dsr_src_table(const dsr_src*, float* table);
/* Carried state (the caller's device memory): per utterance the 64-bit counts of inputs consumed and outputs produced, per (u, c) the last 2K
 * input samples (zoh and linear: ceil(M / L) more, because the count floor(b L / M) can hold back an output whose taps were all there).  init zeroes it and notes its shape in the handle; apply with a state of another shape is DSR_E_CONSISTENCY. */
size_t     dsr_src_state_bytes(const dsr_src*, int U, int C);
dsr_status dsr_src_state_init(dsr_src*, void* state_dev, int U, int C, void* stream);
/* x_dev float [U][C][inStride], nsamp_dev int32 [U] (NULL: inStride each) -> y_dev float [U][C][outStride], nout_dev int32 [U] (optional): the
 * outputs of this call; the rest of a row comes out zero.  state_dev NULL: a one-shot call, floor(nsamp L / M) outputs, outStride at least
 * dsr_src_out_samples(inStride).  With a state the call delivers inputs [a, b) of every stream and produces exactly the outputs not yet produced
 * whose last tap base + K is below b; flush != 0 produces the rest, up to floor(b L / M), with zeros past the end (initialise the state again
 * before the next stream); outStride at least dsr_src_block_out_bound(inStride).  Block by block with a final flush equals the one-shot call bit
 * for bit, whatever the block lengths.  DSR_SRC_TABLE=mem in the environment, read on every call, forces DSR_SRC_TABLE_MEM;
 * DSR_SRC_RUN=n caps the outputs of a tile (256 at the least) and DSR_SRC_TILES=n (1 to 16) sets the tiles a workgroup walks: the tests' switches. */
dsr_status dsr_src_apply(dsr_src*, const float* x_dev, const int32_t* nsamp_dev, int U, int C, int64_t inStride, void* state_dev, int flush,
                         float* y_dev, int32_t* nout_dev, int64_t outStride, void* stream);
/* the cell apply takes: path[0] DSR_SRC_TABLE_*, path[1] DSR_SRC_INPUT_*, path[2] the outputs of a tile, path[3] the launch's dynamic LDS in
 * bytes, path[4] the pitch between the outputs of neighbouring lanes (odd; it spreads their LDS reads over the banks).  The launch takes its decisions from the same helper.  Needs no device. */
dsr_status dsr_src_path(const dsr_src*, int32_t path[5]);
/* measurement (tools/bench_src.py): with timing on, apply brackets its launches with events; kernel_ms waits for them: the last call's ms */
dsr_status dsr_src_set_timing(dsr_src*, int on);
dsr_status dsr_src_kernel_ms(const dsr_src*, double* ms);

/* =====================================================================================
 * 7. Stream/feature-operator API  (FeatureStream<Type,item>::next/reset/size/name/current/isEnd,
 *    btk/stream/stream.h:36-75).  Operators are reference counted handles that hold their
 *    upstream(s); next() returns a pointer to the operator's own output buffer (host memory),
 *    valid until the next call, exactly as the reference's _vector.
 * ===================================================================================== */
typedef struct dsr_stream dsr_stream;
enum { DSR_T_CHAR = 0, DSR_T_SHORT = 1, DSR_T_FLOAT = 2, DSR_T_DOUBLE = 3, DSR_T_COMPLEX = 4 };
dsr_status dsr_stream_next(dsr_stream*, int frameX /* -5 = next */, const void** data, size_t* n);
dsr_status dsr_stream_current(dsr_stream*, const void** data, size_t* n);
dsr_status dsr_stream_reset(dsr_stream*);
int          dsr_stream_size(const dsr_stream*);
int          dsr_stream_type(const dsr_stream*);
int          dsr_stream_frameX(const dsr_stream*);
int          dsr_stream_is_end(const dsr_stream*);
const char*  dsr_stream_name(const dsr_stream*);
void         dsr_stream_retain(dsr_stream*);
void         dsr_stream_release(dsr_stream*);
/* sources */
dsr_status dsr_sample_feature_create(int blockLen, int shiftLen, int padZeros, const char* name, dsr_stream** out);
dsr_status dsr_sample_feature_set_samples(dsr_stream*, const float* samples, size_t n, unsigned sampleRate);
/* SampleFeature::read(fn, format, samplerate, chX, chN, cfrom, to, outsamplerate, norm) (btk/feature/feature.cc:243-393; feature.i:487-489;
 * btk/src/superdirectiveBeamformer.cc:150-247 calls it from C++): RIFF/WAVE PCM of 8/16/24/32 bits; norm == 0 keeps the integer scale, otherwise
 * [-1, 1) x norm; chX is 1-based (0: DSR_E_CONSISTENCY "Multi-channel read is not yet supported."); an empty range or an unreadable file is DSR_E_IO;
 * sample-rate conversion is refused.  *nread = frames read; the stream is reset. */
dsr_status dsr_sample_feature_read(dsr_stream*, const char* fileName, int format, int samplerate, int chX, int chN, int cfrom, int to, int outsamplerate,
                                   float norm, int* nread);
int        dsr_sample_feature_sample_rate(const dsr_stream*);
/* SampleFeature::data() / samplesN() (feature.h): the whole sample buffer, owned by the stream, valid until the next read / setSamples */
dsr_status dsr_sample_feature_data(const dsr_stream*, const float** data, size_t* n);
/* PyFeatureStream equivalent (btk/stream/pyStream.h:44-130): a source whose frames the caller supplies;
   type is DSR_T_SHORT / DSR_T_FLOAT / DSR_T_DOUBLE / DSR_T_COMPLEX, data = nframes rows of `size` items */
dsr_status dsr_frame_source_create(int type, int size, const char* name, dsr_stream** out);
dsr_status dsr_frame_source_set_frames(dsr_stream*, const void* data, size_t nframes);
/* PyFeatureStream::reset() (pyStream.h:100-130) calls the Python object's reset() and iterates it afresh.  A reset() that reaches the source
   through a downstream operator marks its frames stale; `refill(user)` then runs before the next frame is served: it resets the caller's
   iterable and hands the new frames over with dsr_frame_source_set_frames; non-zero return = failure (DSR_E_PYTHON). */
dsr_status dsr_frame_source_set_refill(dsr_stream*, int (*refill)(void* user), void* user);
/* operators (ctor argument order as the reference headers) */
dsr_status dsr_analysis_bank_create(dsr_stream* samp, const double* prototype, int M, int m, int r,
                                    int delayCompensationType, const char* name, dsr_stream** out);
dsr_status dsr_synthesis_bank_create(dsr_stream* samp, const double* prototype, int M, int m, int r,
                                     int delayCompensationType, int gainFactor, const char* name, dsr_stream** out);
/* PerfectReconstructionFFTAnalysisBank(samp, prototype, M, m, r) / ...SynthesisBank(samp, prototype, M, m, r) (modulated.h:377-440) */
dsr_status dsr_pr_analysis_bank_create(dsr_stream* samp, const double* prototype, int M, int m, int r, const char* name, dsr_stream** out);
dsr_status dsr_pr_synthesis_bank_create(dsr_stream* samp, const double* prototype, int M, int m, int r, const char* name, dsr_stream** out);
/* NormalFFTAnalysisBank(samp, M, r, windowType) (modulated.i); samp delivers blocks of D = M >> r samples */
dsr_status dsr_normal_fft_bank_create(dsr_stream* samp, int M, int r, int windowType, const char* name, dsr_stream** out);
/* ZelinskiPostFilter(output, fftLen, alpha, type, minFrames) (postfilter.h:95-126): channels = the snapshot array's analysis
   streams (setSnapShotArray / setBeamformer), manifold = setArrayManifoldVector per bin */
dsr_status dsr_zelinski_stream_create(dsr_stream* output, int fftLen, double alpha, int type, int minFrames, const char* name, dsr_stream** out);
dsr_status dsr_zelinski_stream_set_channel(dsr_stream* pf, dsr_stream* chan);
/* The operators of sections 6a-2 and 6a-3 as streams (postfilter.i:182-428).  Rows are fftLen complex values with the upper half as the reference leaves
 * it.  What the reference objects keep across reset() (noise estimates; Wiener frame counter and PSD memories; the masks' _prevMu) lives as long as the
 * operator; the estimators' reset() clears their accumulators.  An utterance is computed at its first next(), so a control call acts from the next reset().
 * specsub control: 0 setNoiseOverEstimationFactor(value), 1 startTraining, 2 stopTraining, 3 startNoiseSubtraction, 4 stopNoiseSubtraction, 5 clear,
 * 6 clearNoiseSamples, 7 readNoiseFile(fn, idx), 8 writeNoiseFile(fn, idx).  wiener control: 0 setNoiseAmplificationFactor(value), 1 / 2 start /
 * stopUpdatingNoisePSD.  binmask kind as DSR_MASK_*, thest kind as DSR_THEST_*. */
dsr_status dsr_specsub_stream_create(int fftLen, int halfBandShift, float ft, float flooringV, const char* name, dsr_stream** out);
dsr_status dsr_specsub_stream_set_channel(dsr_stream* ss, dsr_stream* chan, double alpha);
dsr_status dsr_specsub_stream_control(dsr_stream* ss, int what, double value, const char* fn, int idx);
dsr_status dsr_wiener_stream_create(dsr_stream* targetSignal, dsr_stream* noiseSignal, int halfBandShift, float alpha, float flooringV, double beta, const char* name,
                                    dsr_stream** out);
dsr_status dsr_wiener_stream_control(dsr_stream* wf, int what, double value);
dsr_status dsr_binmask_stream_create(int kind, unsigned chanX, dsr_stream* srcL, dsr_stream* srcR, unsigned M, float threshold, float alpha, float dEta,
                                     float dPowerCoeff, const char* name, dsr_stream** out);
dsr_status dsr_binmask_stream_set_threshold(dsr_stream* m, float threshold);
dsr_status dsr_binmask_stream_threshold(dsr_stream* m, double* threshold);
dsr_status dsr_binmask_stream_set_thresholds(dsr_stream* m, const double* thresholds, int n);
dsr_status dsr_binmask_stream_thresholds(dsr_stream* m, double* out, int n, int32_t* exists);
dsr_status dsr_thest_stream_create(int kind, dsr_stream* srcL, dsr_stream* srcR, unsigned M, float minThreshold, float maxThreshold, float width, float minFreq,
                                   float maxFreq, int sampleRate, float dEta, float dPowerCoeff, const char* name, dsr_stream** out);
dsr_status dsr_thest_stream_calc_threshold(dsr_stream* e, double* threshold);
dsr_status dsr_thest_stream_threshold(dsr_stream* e, double* threshold);
dsr_status dsr_thest_stream_get_cost_function(dsr_stream* e, unsigned freqX, double* out, size_t outDoubles, size_t* n);
int        dsr_thest_stream_n_cand(dsr_stream* e);      /* the length of getCostFunction() */
dsr_status dsr_thest_stream_thresholds(dsr_stream* e, double* out, int n);
/* McCowanPostFilter(output, fftLen, alpha, type, minFrames, threshold) (postfilter.i:113-126) on the same operator; its noise
   coherence setters: what 0 setNoiseSpatialSpectralMatrix(fbinX, data [C][C] complex), 1 setDiffuseNoiseModel(data = micPos [C][3],
   a = sampleRate, b = sspeed), 2 set(All)Level(s)OfDiagonalLoading(fbinX or -1, a), 3 divideAllNonDiagonalElements(a) */
dsr_status dsr_mccowan_stream_create(dsr_stream* output, int fftLen, double alpha, int type, int minFrames, float threshold, const char* name, dsr_stream** out);
dsr_status dsr_mccowan_stream_set_noise(dsr_stream* pf, int what, int fbinX, const double* data, int chanN, double a, double b);
/* highPassFilter(output, cutOffFreq, sampleRate) (postfilter.h:209-220, postfilter.cc:1222-1261): bins below fftLen*cutOffFreq/sampleRate are cut */
dsr_status dsr_highpass_filter_create(dsr_stream* output, float cutOffFreq, int sampleRate, const char* name, dsr_stream** out);
/* LefkimmiatisPostFilter (postfilter.i, postfilter.h:180-204) on the same operator and setters */
dsr_status dsr_lefkimmiatis_stream_create(dsr_stream* output, int fftLen, double minSV, int fbinX1, double alpha, int type, int minFrames, float threshold,
                                          const char* name, dsr_stream** out);
dsr_status dsr_zelinski_stream_set_manifold(dsr_stream* pf, int fbinX, const double* vec, int chanN);
/* SingleChannelWPEDereverberationFeature(samples, lowerN, upperN, iterationsN, loadDb, bandWidth, sampleRate) (dereverberation.i:67-81) */
dsr_status dsr_wpe_single_stream_create(dsr_stream* samples, int lowerN, int upperN, int iterationsN, double loadDb, double bandWidth,
                                        double sampleRate, const char* name, dsr_stream** out);
/* MultiChannelWPEDereverberation + MultiChannelWPEDereverberationFeature(source, channelX) (dereverberation.i, dereverberation.h:89-174): one
 * operator per channel feature over the source's input streams (setInput order).  All channels of a frame go through the prediction filter
 * of the channel whose feature asks for the frame first (dereverberation.cc:381): by default the feature's own channel; the face that owns
 * the shared source sets the first asker with ..._set_filter_channel (< 0: every channel its own filter). */
dsr_status dsr_wpe_multi_feature_create(dsr_stream* const* channels, int channelsN, int channelX, int lowerN, int upperN, int iterationsN, double loadDb,
                                        double bandWidth, double sampleRate, const char* name, dsr_stream** out);
dsr_status dsr_wpe_multi_feature_set_filter_channel(dsr_stream* feature, int filterChan);
/* NLMS / Kalman / BlockKalman / DTDBlockKalman...EchoCancellationFeature(played, recorded, ...) as a stream (cancelVP.i:62-254) over a dsr_aec
 * handle (not owned; its parameters are read when an utterance is computed).  Serves all fftLen bins, bin fftLen-k = conj(bin k); ends when
 * either upstream ends; a skipped frameX is DSR_E_INDEX, a repeated one returns the cached vector (cancelVP.cc:59-63).  The operator owns its
 * adaptive state and keeps it across reset() as the reference does: NLMS and Kalman zero their filter coefficients, the block variants keep
 * everything.  Unlike the reference, whose reset() forgets to rewind its frame counter (cancelVP.h:60), reset() restarts at frame 0.  DTD: the
 * frameX of the first next() after a reset decides the frame mode of the utterance (< 0: the constant -5).
 *   get: what = DSR_AEC_STATE_* -> out as dsr_aec_state_read with U = 1; *n = the doubles written */
dsr_status dsr_aec_stream_create(dsr_aec* aec, dsr_stream* played, dsr_stream* recorded, const char* name, dsr_stream** out);
dsr_status dsr_aec_stream_get(dsr_stream* s, int what, double* out, size_t outDoubles, size_t* n);
/* CCTDE(samp1, samp2, fftLen, nHeldMaxCC, freqLowerLimit, freqUpperLimit, name) (CCTDE.h:60-101, TDEstimator.i): a stream of double rows, the
 * nHeldMaxCC delays in seconds of a block pair of two SampleFeatures (DSR_E_TYPE otherwise; unequal sampling rates or block sizes and the
 * refusals of dsr_cctde_check are DSR_E_DIMENSION).  fftLen is ignored as there: the transform length is the power of two that holds a block.
 * dsr_stream_next moves both sources on; while they stand at the same frame the rows come from one dsr_cctde_run over the whole utterance.
 *   next_x: nextX(chanX, frameX) -- source chanX moves on, the other one's current block is used again (DSR_E_CONSISTENCY if it has none);
 *   allsamples: the two recordings as one block pair, fftLen < 0 = the power of two that holds the longer one; the result is what
 *               dsr_stream_next(frameX()) and the getters return until a source moves; the transform length stays changed, as there;
 *   get_sample_delays / get_cc_values: the lags as FFT indices (lag >= fftLen/2 stands for lag - fftLen; -1 = empty) and the correlation
 *               values of the last answer, owned by the stream and valid until its next call;
 *   set_target_frequency_range: stored and, as in the reference (CCTDE.cc:186-205 cannot be reached), never used. */
dsr_status dsr_cctde_stream_create(dsr_stream* samp1, dsr_stream* samp2, int fftLen, int nHeldMaxCC, int freqLowerLimit, int freqUpperLimit, const char* name,
                                   dsr_stream** out);
dsr_status dsr_cctde_stream_next_x(dsr_stream* s, int chanX, int frameX, const void** data, size_t* n);
dsr_status dsr_cctde_stream_allsamples(dsr_stream* s, int fftLen);
dsr_status dsr_cctde_stream_get_sample_delays(dsr_stream* s, const int32_t** lags, size_t* n);
dsr_status dsr_cctde_stream_get_cc_values(dsr_stream* s, const double** values, size_t* n);
dsr_status dsr_cctde_stream_set_target_frequency_range(dsr_stream* s, int freqLowerLimit, int freqUpperLimit);
int        dsr_cctde_stream_fft_len(const dsr_stream* s);
/* MCCLocalizer / MCCCalculator as streams (section 2f): setChannel takes any float stream, every channel one block a frame; next() pulls
 * one block from every channel and runs dsr_mcc_run / dsr_mcc_calc with U = B = 1.  The localiser's row is the best position (3 doubles),
 * the calculator's row has the cost in element 0.  Fewer than 2 D samples a block is DSR_E_ERROR "Data samples are insufficient", a
 * calculator without delays DSR_E_ERROR "set time delays with setTimeDelays()", a channel count other than the grid's DSR_E_DIMENSION.
 *   get: what = DSR_MCC_GET_COST (1 double), _TAU (nChan, as doubles), _POSITION (3), _EIGEN (nChan) of the nth best entry of the last
 *        next(); _R (nChan x nChan, nth ignored): getR(). */
#define DSR_MCC_GET_COST     0
#define DSR_MCC_GET_TAU      1
#define DSR_MCC_GET_POSITION 2
#define DSR_MCC_GET_EIGEN    3
#define DSR_MCC_GET_R        4
dsr_status dsr_mcc_stream_create(dsr_mcc* mcc, const char* name, dsr_stream** out);
dsr_status dsr_mcccalc_stream_create(dsr_mcc* mcc, int normalizeVariance, const char* name, dsr_stream** out);
dsr_status dsr_mcc_stream_set_channel(dsr_stream* s, dsr_stream* chan);
dsr_status dsr_mcccalc_stream_set_time_delays(dsr_stream* s, const double* delays, int n);
dsr_status dsr_mcc_stream_get(dsr_stream* s, int what, int nth, double* out, size_t outDoubles, size_t* n);
/* SubbandDS/GSC/MVDR as a stream: channels are analysis-bank streams (setChannel) */
dsr_status dsr_subband_bf_create(dsr_bf* weights, const char* name, dsr_stream** out);
dsr_status dsr_subband_bf_set_channel(dsr_stream* bf, dsr_stream* chan);
/* SubbandMMI as a stream (beamformer.i:255-287): channels through dsr_subband_bf_set_channel; frames beyond fftLen/2 are the conjugate mirror */
dsr_status dsr_subband_mmi_stream_create(dsr_mmi* weights, int fftLen, const char* name, dsr_stream** out);
/* SubbandOrthogonalizer(beamformer, outChanX) (beamformer.h:436-..., beamformer.cc:2817-2849) as a stream over a subband-beamformer operator:
 * outChanX <= 0: the beamformer's output; > 0: column outChanX-1 of the blocking matrices applied to the same snapshots (bins above M/2 as the
 * reference leaves them: the beamformer output's mirror) */
dsr_status dsr_subband_orthogonalizer_create(dsr_stream* beamformer, int outChanX, const char* name, dsr_stream** out);
/* DOAEstimatorSRPDSBLA as a stream (beamformer.i:479-513) over a dsr_doa handle (not owned): channels through dsr_subband_bf_set_channel; next()
 * returns the last direction's beamformed frame, the previous frame's where the energy gate held (bins outside [fbinMin, fbinMax] are never
 * written).  The accumulators survive reset() and are zeroed by a new steering table (after setSearchParam) and by init_accs.
 *   get: what 0 getNBestRPs [nBest], 1 getNBestDOAs [nBest][2], 2 getResponsePowerMatrix [nTheta][1], 3 the accumulators [nTheta],
 *        4 getEnergy [1]; *n = the count written (0 before the first frame for 2 and 3) */
dsr_status dsr_doa_stream_create(dsr_doa* doa, const char* name, dsr_stream** out);
dsr_status dsr_doa_stream_get(dsr_stream* s, int what, double* out, size_t outDoubles, size_t* n);
dsr_status dsr_doa_stream_init_accs(dsr_stream* s);
dsr_status dsr_doa_stream_final_nbest(dsr_stream* s);
/* EigenBeamformer / SphericalDSBeamformer as a stream (beamformer.i:416-455, :551-575) over a dsr_sph handle (not owned): channels through
 * dsr_subband_bf_set_channel; next() returns bins 0..fftLen/2 of y = w^H (sh_s X) and their conjugate mirror (:366-390).
 *   get_eigenbeams: the current frame's eigenbeams F [fftLen/2+1][dim] complex128 (getSnapShotArray) */
dsr_status dsr_sph_bf_stream_create(dsr_sph* sph, const char* name, dsr_stream** out);
dsr_status dsr_sph_stream_get_eigenbeams(dsr_stream* s, double* out, size_t outDoubles, size_t* n);
/* DOAEstimatorSRPEB / DOAEstimatorSRPSphDSB as a stream (beamformer.i:515-550, :601-633) over a dsr_sph handle (not owned), with the pull-by-pull
 * state of dsr_doa_stream_create: next() returns the last unit's bins fbinMin..fbinMax and their mirror, the previous frame's where the gate held;
 * the N-best is reset on every pull; the accumulators survive reset() and are zeroed by a new table and by init_accs.
 *   get: what 0 getNBestRPs [nBest], 1 getNBestDOAs [nBest][2] (theta, phi), 2 getResponsePowerMatrix [nTheta][nPhi], 3 the accumulators
 *        [units], 4 getEnergy [1]; *n = the count written (0 before the first frame for 2 and 3) */
dsr_status dsr_sph_doa_stream_create(dsr_sph* sph, const char* name, dsr_stream** out);
dsr_status dsr_sph_doa_stream_get(dsr_stream* s, int what, double* out, size_t outDoubles, size_t* n);
dsr_status dsr_sph_doa_stream_init_accs(dsr_stream* s);
dsr_status dsr_sph_doa_stream_final_nbest(dsr_stream* s);
/* ModalSphericalArrayTracker / SpatialSphericalArrayTracker as a stream (beamformer.i:880-940, tracker.h:228-236) over a dsr_trk handle (not owned):
 * 32 channels of fftLen complex bins through set_channel; next() returns float (theta, phi).  The filter's state belongs to the operator and
 * outlives reset(); next_speaker = reset() + the initial state (the handle's initial position goes back to (0.5, 0)); set_initial_position moves the
 * position alone.  PlaneWaveSimulator(source, modalDecomposition, channelX, theta, phi) (beamformer.i:942-960, tracker.h:337): rows of fftLen bins. */
dsr_status dsr_trk_stream_create(dsr_trk* trk, const char* name, dsr_stream** out);
dsr_status dsr_trk_stream_set_channel(dsr_stream* s, dsr_stream* chan);
dsr_status dsr_trk_stream_next_speaker(dsr_stream* s);
dsr_status dsr_trk_stream_set_initial_position(dsr_stream* s, double theta, double phi);
dsr_status dsr_pws_stream_create(dsr_stream* source, const dsr_trk* decomposition, unsigned channelX, double theta, double phi, const char* name, dsr_stream** out);
dsr_status dsr_preemphasis_create(dsr_stream* samp, double mu, const char* name, dsr_stream** out);
dsr_status dsr_hamming_create(dsr_stream* samp, const char* name, dsr_stream** out);
dsr_status dsr_fft_create(dsr_stream* samp, int fftLen, const char* name, dsr_stream** out);
dsr_status dsr_spectral_power_create(dsr_stream* fft, int powN, const char* name, dsr_stream** out);
dsr_status dsr_vtln_create(dsr_stream* pow, int coeffN, double ratio, double edge, int version, const char* name, dsr_stream** out);
dsr_status dsr_mel_create(dsr_stream* mag, int powN, float rate, float low, float up, int filterN, int version, const char* name, dsr_stream** out);
dsr_status dsr_log_create(dsr_stream* mel, double m, double a, int sphinxFlooring, const char* name, dsr_stream** out);
dsr_status dsr_cepstral_create(dsr_stream* mel, int ncep, int type, const char* name, dsr_stream** out);
/* WarpMVDRFeature / BurgMVDRFeature (kind 0) and WarpLPCFeature / BurgLPCFeature (kind 1), lpc.h:115-128,280-293 */
dsr_status dsr_lpc_feature_create(dsr_stream* src, int order, int correlate, float warp, int method, int kind, const char* name, dsr_stream** out);
/* WarpedTwiceMVDRFeature(src, order, correlate, warp, warpFactorFixed, sensibility, nm = "WTMVDR") (lpc.h:205-246, lpc.cc:339-357) */
dsr_status dsr_wtmvdr_feature_create(dsr_stream* src, int order, int correlate, float warp, int warpFactorFixed, float sensibility, const char* name,
                                     dsr_stream** out);
/* SpectralSmoothing(adjustTo, adjustFrom, nm = "Spectral Smoothing") (lpc.h:342-358, lpc.cc:473-478): unequal sizes => DSR_E_DIMENSION; the
 * stream ends with the shorter of the two */
dsr_status dsr_spectral_smoothing_create(dsr_stream* adjustTo, dsr_stream* adjustFrom, const char* name, dsr_stream** out);
/* FilterFeature(src, coeffA, nm = "Filter") (feature.h:1315-1410): whole utterances, frame counts as dsr_fir_frames_count */
dsr_status dsr_filter_feature_create(dsr_stream* src, const double* a, int lenA, const char* name, dsr_stream** out);
/* MergeFeature(stat, delta, deltaDelta, nm = "Merge") (feature.h:1423-1441): the three float rows one after the other; ends with the shortest */
dsr_status dsr_merge_feature_create(dsr_stream* stat, dsr_stream* delta, dsr_stream* deltaDelta, const char* name, dsr_stream** out);
/* SamplerateConversionFeature(src, sourcerate = 22050, destrate = 16000, len = 0, method = "fastest", nm = "SamplerateConversion")
 * (feature.h:794-816, feature.cc:1607-1699) over section 6d.  size() is len or, for len 0, unsigned(src.size() * float(destrate) /
 * float(sourcerate)) in float arithmetic (feature.cc:1612).  The source's blocks, one after the other, are the input; the converter is flushed once
 * at the source's end, and the outputs are served in blocks of size(): a last block that cannot be filled is not delivered. */
dsr_status dsr_src_stream_create(dsr_stream* src, unsigned srcRate, unsigned dstRate, unsigned len, const char* method, const char* name,
                                 dsr_stream** out);
/* OverlapAdd(samp, impulseResponse, fftLen = 0, nm = "Overlap Add") / OverlapSave(samp, impulseResponse, nm = "Overlap Save")
 * (convolution.h:40-104): section 2g with C = 1 over the source's blocks; reset() zeroes OverlapAdd's buffer.  update: delta complex[n], n must
 * be L (DSR_E_DIMENSION otherwise, as there); it holds for the utterances materialised after it. */
dsr_status dsr_overlap_add_create(dsr_stream* src, const double* h, int P, int fftLen, const char* name, dsr_stream** out);
dsr_status dsr_overlap_save_create(dsr_stream* src, const double* h, int P, const char* name, dsr_stream** out);
dsr_status dsr_overlap_save_update(dsr_stream* s, const double* delta, int n);
/* The scalar feature operators of section 6c as streams, names and defaults of feature.i (899, 928, 958, 986, 1016, 1148, 1883, 1908, 1936,
 * 1968, 2169).  ALog / Normalize: runon keeps (min, max) across reset() until next_speaker(); SpikeFilter2: reset() sets meanslope = startslope
 * and count = 0 (construction too: the reference leaves both uninitialised), spikes() is the count of the utterance materialised last; verbose is
 * accepted and ignored.  SpectralResampling and SphinxMel work on double streams; powerN 0 takes the source's size. */
dsr_status dsr_signal_power_create(dsr_stream* samp, const char* name, dsr_stream** out);
dsr_status dsr_alog_create(dsr_stream* samp, double m, double a, int runon, const char* name, dsr_stream** out);
dsr_status dsr_normalize_create(dsr_stream* samp, double min, double max, int runon, const char* name, dsr_stream** out);
dsr_status dsr_minmax_next_speaker(dsr_stream* alog_or_normalize);
dsr_status dsr_threshold_create(dsr_stream* samp, double value, double thresh, const char* mode, const char* name, dsr_stream** out);
dsr_status dsr_spectral_resampling_create(dsr_stream* src, double ratio, unsigned len, const char* name, dsr_stream** out);
dsr_status dsr_sphinx_mel_feature_create(dsr_stream* mag, unsigned fftN, unsigned powerN, float sampleRate, float lowerF, float upperF, unsigned filterN,
                                         const char* name, dsr_stream** out);
dsr_status dsr_zcr_hamming_create(dsr_stream* samp, const char* name, dsr_stream** out);
dsr_status dsr_yin_pitch_create(dsr_stream* samp, unsigned samplerate, float threshold, const char* name, dsr_stream** out);
dsr_status dsr_spike_filter_create(dsr_stream* src, unsigned tapN, const char* name, dsr_stream** out);
dsr_status dsr_spike_filter2_create(dsr_stream* src, unsigned width, float maxslope, float startslope, float thresh, float alpha, unsigned verbose, const char* name,
                                    dsr_stream** out);
dsr_status dsr_spike_filter2_spikes(dsr_stream* s, unsigned* n);
dsr_status dsr_amplification_create(dsr_stream* src, double amplify, const char* name, dsr_stream** out);
dsr_status dsr_storage_create(dsr_stream* src, const char* name, dsr_stream** out);
dsr_status dsr_mean_subtraction_create(dsr_stream* src, double devNormFactor, int runon, const char* name, dsr_stream** out);
/* the optional weight stream of MeanSubtractionFeature(src, weight, devNormFactor, runon) (feature.h, feature.cc:2577-2707): element 0 of its frames weighs
 * the frame in the batch statistics; in run-on mode frames with weight <= 0 do not update them */
dsr_status dsr_mean_subtraction_set_weight(dsr_stream* cmn, dsr_stream* weight);
dsr_status dsr_adjacent_create(dsr_stream* single, int delta, const char* name, dsr_stream** out);
dsr_status dsr_linear_transform_create(dsr_stream* src, int sz, const char* name, dsr_stream** out);
dsr_status dsr_linear_transform_set(dsr_stream*, const float* matrix /*[sz][srcSize]*/);
/* LinearTransformFeature::load(fileName, old) (feature.cc:2972-2976): gsl_matrix_float_load + the crop to (size x srcSize) */
dsr_status dsr_linear_transform_load(dsr_stream*, const char* fileName, int old);
/* StorageFeature::write(fileName, plainText) / read(fileName) (feature.cc:3025-3067), quirks kept (the count written is the index of the last
   frame; read() loads that many frames, one fewer than the file holds) */
dsr_status dsr_storage_write(dsr_stream*, const char* fileName, int plainText);
dsr_status dsr_storage_read(dsr_stream*, const char* fileName);

/* On-disk formats either side of the path, host side.
 * gsl_matrix_float_load / gsl_vector_float_load(m, fileName, old) (btk/matrix/gslmatrix.cc:27-96,133-240) into a caller matrix of rows x cols:
 *   old == 0: the GSL raw block (rows*cols native-endian floats); old != 0: Janus "FMAT"/"FVEC" (magic, big-endian sizes, a count that is
 *   skipped, big-endian floats; rows < 0 = derived from the file length).  Errors as the reference raises them: DSR_E_IO "Couldn't find magic
 *   number", "File empty", "Number of bytes in file = don't match matrix dimension"; DSR_E_DIMENSION "Cannot resize" when the file's matrix is
 *   larger than the caller's.  *rowsOut x *colsOut: the matrix size after the load (the file's, for old != 0). */
dsr_status dsr_fmat_load(const char* fileName, int old, int rows, int cols, float* data, int* rowsOut, int* colsOut);
dsr_status dsr_fmat_save(const char* fileName, int old, int rows, int cols, const float* data, int rowsUnset);
dsr_status dsr_fvec_load(const char* fileName, int old, int n, float* data, int* nOut);
dsr_status dsr_fvec_save(const char* fileName, int old, int n, const float* data);
/* HTK parameter files (btk/feature/feature.cc:4025-4318: ReadHTKHeader / WriteHTKHeader / ReadFloatBinary / WriteFloatBinary,
 * WriteHTKFeatureFile, HTKFeature): 12-byte header + float vectors of sampSize bytes.  isBigEndian is the reference's flag ("the machine is big
 * endian"): when 0 every field is byte-swapped, which gives the big-endian files HTK expects.  Compressed (_C) and CRC (_K) kinds: DSR_E_IO. */
dsr_status dsr_htk_write(const char* fileName, int nSamples, int sampPeriod, int sampSize, int parmKind, int isBigEndian, const float* data);
dsr_status dsr_htk_read_header(const char* fileName, int isBigEndian, int* nSamples, int* sampPeriod, int* sampSize, int* parmKind);
dsr_status dsr_htk_read(const char* fileName, int isBigEndian, float* data, size_t nFloats);

/* =====================================================================================
 * 7b. Speech activity detection, btk/sad/sad.{h,cc} (csrc/k_sad.hip; line numbers are sad.cc's)
 *
 * Batch entries take device arrays [U][Tmax][...], nframes_dev int32 [U] (NULL: Tmax frames each) and a stream.  Frames at or past an
 * utterance's count are never read; their outputs are zero.  Every metric returns a decision [U][Tmax] fp64 (the value next() returns) and a
 * score [U][Tmax] fp64.  A metric with carried state is a function (input, nframes, state in) -> (outputs, state after nframes frames): the
 * state arrays are read and written in place, and two calls that carry them equal one call.
 * ===================================================================================== */
/* EnergyVADMetric (:438-554).  score = the frame's energy, an fp64 sum of squares of the widened floats, i ascending (:486-490); decision 1.0
 * where it exceeds sorted[unsigned(threshold * energiesN)] of the history, else 0.0 -- evaluated as "more than that many history entries are
 * below it", without a sort.  hist_dev fp64 [U][energiesN] is a ring (the history's order never decides anything); counters_dev int32 [U][4] =
 * (aboveThresholdN, belowThresholdN, recognizing, ring position).  The history takes the frame's energy only while !recognizing &&
 * aboveThresholdN == 0, tested before the frame's counters change (:495); updates_dev (may be NULL) int32 [U] counts those frames.
 * state_init fills the history with initialEnergy and clears the counters (nextSpeaker, :465-472); countersOnly != 0 clears
 * (aboveThresholdN, belowThresholdN, recognizing) alone (reset, :459-463: the history survives).  threshold outside [0, 1) indexes one past the
 * sorted array in the reference: DSR_E_DIMENSION; energiesN outside [1, 8192] likewise. */
dsr_status dsr_sad_energy_state_init(double* hist_dev, int32_t* counters_dev, int U, int energiesN, double initialEnergy, int countersOnly, void* stream);
dsr_status dsr_sad_energy_run(const float* x_dev, const int32_t* nframes_dev, int U, int Tmax, int dim, double threshold, unsigned headN, unsigned tailN, int energiesN,
                              double* hist_dev, int32_t* counters_dev, double* decision_dev, double* score_dev, int32_t* updates_dev, void* stream);
/* EnergyVADMetric::energyPercentile (:510-519) of one utterance's history on the host: sorted[int(percentile / 100 * energiesN)] / energiesN.
 * percentile outside [0, 100] as there; 100 reads one past the array there: DSR_E_DIMENSION. */
dsr_status dsr_sad_energy_percentile(const double* hist_host, int energiesN, double percentile, double* value);
/* SimpleEnergyVAD::next (:174-194): X_dev complex128 [U][Tmax][fftLen]; e = sum_k |X[k]|^2 over all fftLen bins, E <- gamma E + (1 - gamma) e,
 * score = e / E, decision 1.0 where it exceeds threshold else 0.0.  E_dev fp64 [U] is the carried state (0 after nextSpeaker, :168-171). */
dsr_status dsr_sad_simple_energy_run(const void* X_dev, const int32_t* nframes_dev, int U, int Tmax, int fftLen, double threshold, double gamma, double* E_dev,
                                     double* decision_dev, double* score_dev, void* stream);
/* MultiChannelVADMetric::_setLowX / _setHighX / _setBinN (:595-629); a cutoff < 0 means none, one >= sampleRate / 2 is DSR_E_DIMENSION */
dsr_status dsr_sad_band(unsigned fftLen, double sampleRate, double lowCutoff, double highCutoff, unsigned* lowX, unsigned* highX, unsigned* binN);
/* PowerSpectrumVADMetric (kind 0, :660-705), NormalizedEnergyMetric (1, :743-796), TSPSVADMetric (2, :972-1024).  P_dev float
 * [U][C][Tmax][fftLen/2+1]; channel 0 is the target.  powers_dev fp64 [U][Tmax][C] (getMetrics()) = the fp64 sum over lowX .. highX ascending,
 * bin 0 with weight 1 and every other bin, the Nyquist bin too, with weight 2 (fbinX == _fftLen2 + 1 is never true inside the loop), / fftLen.
 * score = p0 / sum p | sqrt p0 / sum sqrt p | log(p0 / (sum p - p0)) - log(E0 / sum p); decision +-1.0: score > E0 / C (kinds 0, 1), > 0 (2). */
dsr_status dsr_sad_power_run(const float* P_dev, const int32_t* nframes_dev, int U, int C, int Tmax, unsigned fftLen, unsigned lowX, unsigned highX, int kind, double E0,
                             double* decision_dev, double* powers_dev, double* score_dev, void* stream);
/* CCCVADMetric::next (:842-941).  X_dev complex64 (isDouble 0) or complex128 [U][C][Tmax][fftLen].  Per frame a buffer of fftLen complex fp64
 * is cleared once (:855); for c = 1 .. C-1 in order the PHAT-normalised cross spectrum conj(X0) Xc / |conj(X0) Xc| goes to bins lowX .. highX
 * and their mirrors, the buffer is transformed in place (inverse radix 2, times 1 / fftLen) and the n-best pass runs over its real parts.  Kept
 * as written: the buffer is not cleared between channels, and in the insertion loop (:887-903) a value above the last candidate always lands
 * in slot 0, the others moving down only if it also exceeds slot 0.  score = the mean over the channels of the mean of the nCand slots;
 * decision 1.0 where score < threshold else -1.0 (a silent frame: NaN and -1.0).  cands_dev (may be NULL) fp64 [U][Tmax][nCand]: the slots as
 * the last channel leaves them (getMetrics()).  fftLen no power of two in [4, 2048], nCand outside [1, 64],
 * C < 2: DSR_E_DIMENSION. */
dsr_status dsr_sad_ccc_run(const void* X_dev, int isDouble, const int32_t* nframes_dev, int U, int C, int Tmax, unsigned fftLen, unsigned lowX, unsigned highX,
                           unsigned nCand, double threshold, double* decision_dev, double* score_dev, double* cands_dev, void* stream);
/* DIAGNOSTIC entry, for tools/bench_sad.py only; its score is no metric.  The same kernel without the n-best pass (score = the mean over the channels of sample 0), so that the pass's share of
 * the time can be taken as a difference */
dsr_status dsr_sad_ccc_transforms_only(const void* X_dev, int isDouble, int U, int C, int Tmax, unsigned fftLen, unsigned lowX, unsigned highX, double* decision_dev,
                                       double* score_dev, void* stream);
/* NegentropyVADMetric (kind 0, :1103-1142), MutualInformationVADMetric (1, :1437-1535), LikelihoodRatioVADMetric (2, :1572-1628).
 * The model lives on the host (std::lgamma / std::tgamma): per bin the shape factor f, Bc and the normalisation of the marginal generalised
 * Gaussian (:1038-1049), and with joint != 0 the matched joint shape factor of the bisection _match (:1338-1369), its Bc and normalisation
 * (:1229-1246) and the fixed part of the decision threshold (:1399-1434).  The reference loops for ever where _match does not converge: here 200
 * steps, then DSR_E_NUMERIC.  shapeFactors: fftLen/2+1 host doubles (NULL: all 2.0, the Gaussian); read_shape_factors takes them from the
 * reference's directory of _M-%04d files, second token of the first line (:1077-1095).  table: [fftLen/2+1][6] = (f, Bc, norm, fJ, BJ, normJ).
 * run: X1 / X2 complex128 [U][Tmax][fftLen], env1 / env2 float [U][Tmax][envDim], envDim >= fftLen/2+1 (kind 0 reads X1 and env1 only).  The
 * device does the per-bin fp64 work (pow, log, the 2x2 quadratic form of :1253-1284 written out) and the weighted sum over lowX .. highX
 * ascending (only bin 0 has weight 1), / binN.  score = that sum; decision 1.0 where score > threshold else 0.0.  kind 1 carries rho_dev
 * complex128 [U][fftLen/2+1]: used before it is updated (:1479, :1504-1510), rescaled to 0.9 where |rho| >= 0.9, zero after nextSpeaker() only;
 * twiddle < 0 compares with `threshold`, otherwise with _calcTotalThreshold (:1437-1454) of the rho before the frame; threshold_dev (may be NULL)
 * [U][Tmax] receives the threshold each frame was compared with.  kind 2 uses sqrt((env1 + env2) / 2) of the unrooted envelopes, as written
 * (:1594-1599).  The reference's per-frame printfs are dropped. */
typedef struct dsr_sad_gg dsr_sad_gg;
dsr_status dsr_sad_gg_create(const double* shapeFactors, unsigned fftLen, double sampleRate, double lowCutoff, double highCutoff, int joint, dsr_sad_gg** out);
void       dsr_sad_gg_destroy(dsr_sad_gg*);
dsr_status dsr_sad_gg_table(const dsr_sad_gg*, double* table, double* fixedThreshold);
dsr_status dsr_sad_gg_read_shape_factors(const char* directory, unsigned fftLen, double* shapeFactors);
dsr_status dsr_sad_gg_run(dsr_sad_gg*, int kind, const void* X1_dev, const void* X2_dev, const float* env1_dev, const float* env2_dev, int envDim,
                          const int32_t* nframes_dev, int U, int Tmax, double twiddle, double threshold, double beta, void* rho_dev, double* decision_dev,
                          double* score_dev, double* threshold_dev, void* stream);
/* The segmenters' rule, HangoverVADFeature::next (:1767-1837), over K metrics' decisions fp64 [K][U][Tmax]: wait for headN consecutive source
 * frames above threshold, emit from the oldest buffered one, end before the tailN-th consecutive frame below, or where the source ends.
 * kind 0: HangoverVADFeature (decision 0 > thresholds[0], :1756-1765); 1: HangoverMIVADFeature (K = 3, codes -1, 2, 3, -3, :1853-1879);
 * 2: HangoverMultiStageVADFeature (:1904-1945; K < 3 is never above).  thresholds: K host doubles.  Per utterance: start = _prefixN - headN,
 * the first emitted source frame (nframes - headN when the utterance never starts); length, 0 for one that never starts; consumed, the source
 * frames the reference would have pulled; decision_metric_dev int32 [U][Tmax], _decisionMetric after each pulled source frame (0 for kind 0).
 * The metrics' decisions are those of a walk over all nframes frames; the reference never evaluates a metric past `consumed`, so a caller
 * that carries a metric's state runs that metric again with nframes = consumed from the state it started with. */
dsr_status dsr_sad_hangover_run(const double* decisions_dev, const int32_t* nframes_dev, int K, int U, int Tmax, const double* thresholds, unsigned headN, unsigned tailN,
                                int kind, int32_t* start_dev, int32_t* length_dev, int32_t* consumed_dev, int32_t* decision_metric_dev, void* stream);
/* y [U][Tmax][dim]: row j of utterance u = row start[u] + j of x for j < length[u], zeros after */
dsr_status dsr_sad_gather_run(const float* x_dev, const int32_t* start_dev, const int32_t* length_dev, int U, int Tmax, int dim, float* y_dev, void* stream);

/* The spectral-shape operators of btk/sad/sadFeature.cc, y float [U][Tmax][1].  op 0 EnergyDiffusionFeature (:93-118): -sum nval log10(nval) over
 * nval = x / |x| > 0 in fp64; 1 BandEnergyRatioFeature (:129-153): sqrt(ssLow / ssHigh), float sums of squares below and from bin
 * int(floor(threshF / (sampleRate / 2 / dim))), threshF <= 0 meaning sampleRate / 4 (thresh carries threshF; band_ratio_index returns the bin, and
 * DSR_E_DIMENSION where it lies past the frame, which the reference would read); 2 NegativeEntropyFeature (:205-243): 100 (E ln cosh z - 0.374576)^2
 * of the rectified frame normalised to zero mean and unit variance, z rounded to float as there, ln and cosh in fp64; 3 SignificantSubbandsFeature
 * (:253-274): the count of x / sigma > thresh, sigma the float norm() result widened again (:27-39). */
dsr_status dsr_sad_band_ratio_index(int dim, float sampleRate, float threshF, int* threshX);
dsr_status dsr_sad_shape_run(const float* x_dev, const int32_t* nframes_dev, int U, int Tmax, int dim, int op, float sampleRate, float thresh, float* y_dev, void* stream);

/* The metrics and segmenters over streams, names and defaults of sad.i.  A metric materialises its sources' utterance at the first next() after
 * a reset() and serves frame frameX of the batch result (frameX < 0: the next one); DSR_E_ITERATOR past the end.  reset() commits the carried
 * state of the frames served so far (an EnergyVADMetric keeps its history, :459-463) and resets the sources; next_speaker() refills it.
 * A segmenter is a float stream; it commits its stateful metrics with the frames it consumed.  In HangoverMultiStageVADFeature the reference
 * calls a metric at stage >= 2 twice in a frame where that stage fires (:1932-1935), which advances a stateful metric twice: an
 * EnergyVADMetric or MutualInformationVADMetric there is refused with DSR_E_CONSISTENCY (a SimpleEnergyVAD handle too). */
typedef struct dsr_vad_metric dsr_vad_metric;
dsr_status dsr_sad_energy_metric_create(dsr_stream* source, double initialEnergy, double threshold, unsigned headN, unsigned tailN, unsigned energiesN, const char* name,
                                        dsr_vad_metric** out);
dsr_status dsr_sad_power_metric_create(int kind, unsigned fftLen, double sampleRate, double lowCutoff, double highCutoff, const char* name, dsr_vad_metric** out);
dsr_status dsr_sad_ccc_metric_create(unsigned fftLen, unsigned nCand, double sampleRate, double lowCutoff, double highCutoff, const char* name, dsr_vad_metric** out);
dsr_status dsr_sad_simple_energy_create(dsr_stream* samp, double threshold, double gamma, dsr_vad_metric** out);
/* kind as dsr_sad_gg_run; source2 / spectralEstimator2 are NULL for kind 0; shapeFactorDir "" or NULL: all 2.0; the spectral estimators are any
 * float streams of at least fftLen/2+1 elements.  fftLen = the size of source1.  nextSpeaker() zeroes rho (:1543-1550), reset() keeps it. */
dsr_status dsr_sad_gg_metric_create(int kind, dsr_stream* source1, dsr_stream* source2, dsr_stream* spectralEstimator1, dsr_stream* spectralEstimator2,
                                    const char* shapeFactorDir, double twiddle, double threshold, double beta, double sampleRate, double lowCutoff, double highCutoff,
                                    const char* name, dsr_vad_metric** out);
void       dsr_sad_metric_release(dsr_vad_metric*);
dsr_status dsr_sad_metric_set_channel(dsr_vad_metric*, dsr_stream* chan);
dsr_status dsr_sad_metric_clear_channel(dsr_vad_metric*);
dsr_status dsr_sad_metric_set_e0(dsr_vad_metric*, double E0);
dsr_status dsr_sad_metric_set_ncand(dsr_vad_metric*, unsigned nCand);
dsr_status dsr_sad_metric_set_threshold(dsr_vad_metric*, double threshold);
dsr_status dsr_sad_metric_next(dsr_vad_metric*, int frameX, double* value);
dsr_status dsr_sad_metric_reset(dsr_vad_metric*);
dsr_status dsr_sad_metric_next_speaker(dsr_vad_metric*);
dsr_status dsr_sad_metric_score(dsr_vad_metric*, double* score);
dsr_status dsr_sad_metric_powers(dsr_vad_metric*, double* powers, int n);
dsr_status dsr_sad_metric_energy_percentile(dsr_vad_metric*, double percentile, double* value);
/* kind as dsr_sad_hangover_run.  add_metric: the further metrics of HangoverMIVADFeature's constructor and HangoverMultiStageVADFeature::setMetric */
dsr_status dsr_sad_hangover_create(dsr_stream* source, dsr_vad_metric* metric, double threshold, unsigned headN, unsigned tailN, int kind, const char* name,
                                   dsr_stream** out);
dsr_status dsr_sad_hangover_add_metric(dsr_stream* hangover, dsr_vad_metric* metric, double threshold);
dsr_status dsr_sad_hangover_next_speaker(dsr_stream* hangover);
dsr_status dsr_sad_hangover_prefix_n(dsr_stream* hangover, int* prefixN);
dsr_status dsr_sad_hangover_decision_metric(dsr_stream* hangover, int* decisionMetric);
/* EnergyDiffusionFeature(src, nm), BandEnergyRatioFeature(src, sampleRate, threshF, nm), NegativeEntropyFeature(src, nm),
 * SignificantSubbandsFeature(src, thresh, nm) (sadFeature.h): op as dsr_sad_shape_run, one value a frame */
dsr_status dsr_sad_shape_create(dsr_stream* src, int op, float sampleRate, float thresh, const char* name, dsr_stream** out);

/* =====================================================================================
 * 8. The distribution set as the decoder sees it
 *    replaces Distrib::score(frameX) (asr/gaussian/distribBasic.h:48-50), DistribSet::find (:183-190), resetCache / resetFeature (:177-178) and
 *    the pull chain decoder -> distribution -> codebook -> feature stream (decoder.h:985, codebookBasic.cc:431-465): a GMM model bound to a
 *    feature-stream handle.  score() pulls frame frameX through the stream protocol (DSR_E_ITERATOR at the end, DSR_E_INDEX out of order), scores
 *    every distribution of that frame on the device once and serves the frame's other requests from that (the reference caches per codebook and
 *    frame).  decode_stream() = _Decoder::decode() for the utterance the stream holds: features, scores and token passing stay on the device.
 * ===================================================================================== */
typedef struct dsr_distribset dsr_distribset;
dsr_status dsr_distribset_create(dsr_gmm*, dsr_stream* feature, int gmmMode /* as dsr_gmm_score */, dsr_distribset** out);
void       dsr_distribset_destroy(dsr_distribset*);
int        dsr_distribset_ndists(const dsr_distribset*);
dsr_status dsr_distribset_find(const dsr_distribset*, const char* name, int* distX);
const char* dsr_distribset_name(const dsr_distribset*, int distX);
dsr_status dsr_distribset_score(dsr_distribset*, int distX, int frameX, float* score);
dsr_status dsr_distribset_reset_cache(dsr_distribset*);
dsr_status dsr_distribset_reset_feature(dsr_distribset*);
dsr_status dsr_decoder_decode_stream(dsr_decoder*, dsr_distribset*, dsr_decode_result* res, int32_t* arcs_out, uint32_t* words_out, int maxPath);
/* Lattice::gammaProbsDist(dss, acScale, lmScale, lmPenalty, silPenalty, silSymbol) (asr/lattice/lattice.cc:331-341, 381-409): the acoustic score of
 * every link with an input symbol that leaves the initial node or a node of _nodes becomes the sum of its distribution's scores over the link's
 * frames (double accumulator, frame order; the frames of the bound feature stream are scored on the device, the sums are one gather kernel), then
 * gammaProbs.  DSR_E_INDEX: a link names a distribution or a frame the set / the stream does not have. */
dsr_status dsr_lattice_gamma_probs_dist(dsr_lattice*, dsr_distribset*, double acScale, double lmScale, double lmPenalty, double silPenalty,
                                        unsigned silenceX, double* logProb);

/* =====================================================================================
 * 8b. Multi-stream decoding: two acoustic models at once (csrc/ms_kernels.hip, csrc/multistream.cpp)
 *    replaces DistribMultiStream (asr/gaussian/distribBasic.h:135-158), DistribMap (distribBasic.h:390-408, distribBasic.cc:326-376) and
 *    DistribSetMultiStream (distribBasic.cc:381-417).  Every state's cost is
 *        float(audioWeight * double(audio score) + videoWeight * double(video score))         (distribBasic.h:148-152)
 *    -- two fp64 products, one fp64 sum, one rounding, no fused multiply-add -- where the video state of audio state `name` is
 *    videoSet.find(name), or videoSet.find(map.mapped(name)) with a map; many audio states may share one video state.  The two streams need not
 *    be audio and video: MFCC plus warped-MVDR cepstra, array output plus a close-talk channel.  More than two streams, weight estimation and
 *    training through a multi-stream set are not built.
 * ===================================================================================== */
/* DistribMap (distribBasic.h:390-408): names of the first model -> names of the second.  Host only, needs no device.  The reference reads names into
 * char[20] (distribBasic.cc:338-339): a name of more than 19 characters is DSR_E_PARAMETER on add, read and write instead of an overflow. */
typedef struct dsr_distribmap dsr_distribmap;
dsr_status dsr_distribmap_create(dsr_distribmap** out);
void       dsr_distribmap_destroy(dsr_distribmap*);
dsr_status dsr_distribmap_add(dsr_distribmap*, const char* from, const char* to);                /* distribBasic.h:398: a later add overwrites */
/* distribBasic.cc:349-357: DSR_E_INDEX "No mapping for %s"; *to is valid until the map changes */
dsr_status dsr_distribmap_mapped(const dsr_distribmap*, const char* name, const char** to);
int        dsr_distribmap_size(const dsr_distribmap*);
/* distribBasic.cc:326-347, 359-376 with read_string / write_string (btk/common/mach_ind_io.cc:490-500, 1009-1021): a big-endian int32 count, then
 * per pair two strings, each a big-endian int16 length and length + 1 bytes, in std::map key order.  read clears the map first.  An empty file
 * name is DSR_E_ERROR "Distribution map file name is null.", a file that cannot be opened DSR_E_IO. */
dsr_status dsr_distribmap_read(dsr_distribmap*, const char* fileName);
dsr_status dsr_distribmap_write(const dsr_distribmap*, const char* fileName);

/* The combiner of two models' score matrices.  create resolves every audio name to the index of its video state once -- the constructors'
 * loops, distribBasic.cc:385-391, 400-409: DSR_E_KEY for a name the video model lacks, DSR_E_INDEX for a name the map lacks (map NULL: by name)
 * -- and keeps the table [KA] on the device.  Default weights of the reference: 0.95 / 0.05 (distribBasic.h:137); they need not sum to one. */
typedef struct dsr_ms dsr_ms;
dsr_status dsr_ms_create(const dsr_gmm* audio, const dsr_gmm* video, const dsr_distribmap* map, double audioWeight, double videoWeight, dsr_ms** out);
void       dsr_ms_destroy(dsr_ms*);
dsr_status dsr_ms_set_weights(dsr_ms*, double audioWeight, double videoWeight);                   /* distribBasic.h:142-145, for the next combine */
dsr_status dsr_ms_get_weights(const dsr_ms*, double* audioWeight, double* videoWeight);           /* distribBasic.h:140-141 */
dsr_status dsr_ms_table(const dsr_ms*, int32_t* table /* host [KA] */);
/* DistribMultiStream::_score (distribBasic.h:148-152) for N frames x KA states: sA_dev [N][KA], sV_dev [N][KV] fp32 costs (dsr_gmm_score of the two
 * models) -> out_dev [N][KA].  out_dev may be sA_dev itself; otherwise it is disjoint from both inputs, and it never aliases sV_dev.  N == 0 does
 * nothing. */
dsr_status dsr_ms_combine(dsr_ms*, const float* sA_dev, const float* sV_dev, int64_t N, float* out_dev, void* stream);
/* Which k_ms_combine the call launches, a pure function of the shapes and of whether sA_dev and out_dev are both 16-byte aligned; the launch asks
 * the same helper.  rowsPerTile consecutive rows are one workgroup's tile, ldsBytes its dynamic LDS.  Needs no device. */
enum { DSR_MS_VECTOR_LDS = 0,          /* KA % 4 == 0 and aligned: float4 audio accesses, the tile's video rows in LDS */
       DSR_MS_SCALAR_LDS = 1,          /* any KA, any 4-byte alignment: 4-byte audio accesses, the video rows still in LDS */
       DSR_MS_GATHER = 2 };            /* 4 KV > DSR_MS_LDS_BUDGET, one video row alone exceeds the budget: sV[n][map[k]] read from memory */
enum { DSR_MS_LDS_BUDGET = 32768 };    /* bytes of LDS a tile's video rows may take */
dsr_status dsr_ms_combine_path(int KA, int KV, int aligned16, int* path, int* rowsPerTile, int64_t* ldsBytes);

/* DistribSetMultiStream(audioDistSet, videoDistSet[, distribMap], audioWeight, videoWeight) (distribBasic.cc:381-410) as a dsr_distribset that every
 * entry of section 8 accepts.  ndists / find / name are the audio set's; reset_cache / reset_feature reach both children; score(distX, frameX)
 * pulls frame frameX of BOTH children through the stream protocol (DSR_E_ITERATOR when either stream has ended, DSR_E_INDEX out of order) and
 * combines the two rows with dsr_ms_combine's kernel; decode_stream materialises both streams, scores T = min(T_audio, T_video) frames of each in
 * the child's own mode, combines on the device in place and decodes (T == 0: DSR_E_ITERATOR); gamma_probs_dist uses the combined matrix.  Each
 * child keeps its own feature stream, dimension and scoring mode.  The children are plain sets (DSR_E_TYPE otherwise); the new set retains them,
 * destroying it releases them, and they stay usable on their own.  The constructor errors are dsr_ms_create's. */
dsr_status dsr_distribset_create_multistream(dsr_distribset* audioSet, dsr_distribset* videoSet, const dsr_distribmap* map /* NULL: by name */,
                                             double audioWeight, double videoWeight, dsr_distribset** out);
/* DistribSetMultiStream::setWeights (distribBasic.cc:412-417); DSR_E_TYPE on a plain set */
dsr_status dsr_distribset_set_weights(dsr_distribset*, double audioWeight, double videoWeight);
dsr_status dsr_distribset_get_weights(const dsr_distribset*, double* audioWeight, double* videoWeight);

/* =====================================================================================
 * 9. GMM training: ML / MMI accumulation, updates, accumulator files
 *    replaces CodebookTrain / CodebookSetTrain (asr/train/codebookTrain.cc, "cT"), DistribTrain / DistribSetTrain / AccMap
 *    (asr/train/distribTrain.cc, "dT") for the diagonal 1:1 models dsr_gmm holds.  One item = DistribTrain::accumulate(frameX, factor)
 *    (dT:74-80): posteriors of the frame under the distribution (_scoreAll, codebookBasic.cc:645-766, then the normalisation of cT:100-105),
 *    gamma = posterior * factor (float), then count / denCount / sumO / sumOsq of the codebook (cT:520-540, 354-358) and count / denCount of the
 *    distribution (dT:133-142), all fp64.  The posteriors and gammas are computed per item exactly in the reference's order; the sums OVER
 *    ITEMS are formed by an fp64 MFMA contraction in a fixed order (the same call twice gives the same bits; no atomics), so they differ from
 *    the reference's sequential sums by fp64 reordering and by the float roundings of x*gamma and (gamma*x)*x, which the contraction skips.
 *    Deviations: MinimumCount (cT:458,590: a process-wide static) belongs to the handle; an item whose posterior sum is zero or not finite --
 *    the reference divides by it and accumulates NaN -- is refused like a NaN score; shared codebooks do not arise (1:1 models).
 *    The handle keeps the dsr_gmm it was made from (which must outlive it) and CHANGES it in update / split; every such entry re-uploads the
 *    device copies of the model, so scoring in any mode sees the new parameters, and dsr_gmm_save writes the trained model.
 *    (nParts, part) select codebooks / distributions as List::Iterator(lst, nParts, part) does (btk/common/mlist.h:155-178); 1, 1 = all.
 * ===================================================================================== */
typedef struct dsr_train dsr_train;
/* CodebookSetTrain(descFile, fs, cbkFile, massThreshold) (cT:586-599) + allocAccus (cT:617-623) + DistribSetTrain (dT:424-437): zeroed accumulators */
dsr_status dsr_train_create(dsr_gmm*, double massThreshold, dsr_train** out);
void       dsr_train_destroy(dsr_train*);
/* zeroAccus (cT:688-694, dT:491-497); what: 1 codebook accumulators, 2 distribution accumulators, 3 both */
dsr_status dsr_train_zero(dsr_train*, int what, int nParts, int part);
int        dsr_train_num_gaussians(const dsr_train*);
/* The batch entry: M items (frame[i], dist[i], factor[i]) over x_dev [N][dimN] fp32 (host index arrays).  score [M] or NULL: the float score of
 * every item (cT:95).  DSR_E_INDEX: a frame outside [0, N) or a distribution outside the set; DSR_E_NUMERIC: an item's score is NaN (cT:97-98)
 * or its posterior sum is zero / not finite -- nothing of the call is then applied.  The call returns when the sums are on the device. */
dsr_status dsr_train_accumulate(dsr_train*, const float* x_dev, int64_t N, const int32_t* frame, const int32_t* dist, const float* factor, int64_t M,
                                float* score, void* stream);
/* DistribSetTrain::accumulate(path, factor) (dT:515-526): frame t with distribution distIds[t]; *score = the double sum of the float scores */
dsr_status dsr_train_accumulate_path(dsr_train*, const float* x_dev, int64_t T, const int32_t* distIds, float factor, double* score, void* stream);
/* DistribSetTrain::accumulateLattice(lat, factor) (dT:528-561) with the lattice's current gammas (call gamma_probs first): links with input 0 or
 * gamma > 10 are skipped, the others give postProb = float(factor exp(-gamma)) for frames start..end of distribution input - 1; *linksN = the
 * reference's "links" count.  DSR_E_INDEX: start < 0, end >= T or an input beyond the set. */
dsr_status dsr_train_accumulate_lattice(dsr_train*, dsr_lattice*, const float* x_dev, int64_t T, float factor, unsigned* linksN, void* stream);
/* for callers without a HIP binding of their own (host/dsr_streams.hpp): N frames of dimN floats from host memory into a buffer the handle
 * owns; *x_dev stays valid until the next upload or the handle's end */
dsr_status dsr_train_upload_features(dsr_train*, const float* x_host, int64_t N, const float** x_dev);
/* The six accumulators as fp64 (any pointer may be NULL): count, denCount [G], sumO, sumOsq [G][dimN] of the codebooks, count, denCount [G] of the
 * distributions; G = sum of refN, Gaussians in model order */
dsr_status dsr_train_get(dsr_train*, double* count, double* denCount, double* sumO, double* sumOsq, double* distCount, double* distDenCount);
dsr_status dsr_train_set(dsr_train*, const double* count, const double* denCount, const double* sumO, const double* sumOsq, const double* distCount,
                         const double* distDenCount);
/* Accu::add (cT:392-405: scaled by factor) and DistribTrain::Accu::add (dT:254-262: factor ignored, as written) */
dsr_status dsr_train_add(dsr_train*, dsr_train* other, double factor);
/* CodebookSetTrain::saveAccus / loadAccus (cT:625-678, Accu::save/load :299-433, AccMap dT:343-419) and DistribSetTrain::saveAccus / loadAccus
 * (dT:439-489, Accu::save/load :239-312): big-endian; loading ADDS factor x the stored floats; names absent from the file's map are skipped;
 * a size mismatch is DSR_E_DIMENSION, a wrong marker DSR_E_IO (codebooks) / DSR_E_ERROR (distributions) */
dsr_status dsr_train_save_codebook_accus(dsr_train*, const char* fileName, float totalPr, unsigned totalT, int countsOnly);
dsr_status dsr_train_load_codebook_accus(dsr_train*, const char* fileName, float* totalPr, unsigned* totalT, float factor, int nParts, int part);
dsr_status dsr_train_save_distrib_accus(dsr_train*, const char* fileName);
dsr_status dsr_train_load_distrib_accus(dsr_train*, const char* fileName, float factor, int nParts, int part);
/* Updates of the model (host arithmetic in the reference's order and precision).  what: 1 codebooks, 2 distributions, 3 both.
 *   update            Accu::update (cT:435-490: count, mean, then VARIANCES in the model's covariance slot) / DistribTrain::Accu::update (dT:146-156)
 *   update_mmi        Accu::updateMMI (cT:442-446,492-518) / DistribTrain::Accu::updateMMI (dT:158-222; DSR_E_CONSISTENCY as the reference throws)
 *   floor_variances   CodebookTrain::floorVariances (cT:786-798, floor 1e-4): adds to *total and *floored
 *   fix_gconsts       GaussDensity::fixGConst (cT:228-241); DSR_E_CONSISTENCY when a determinant is NaN
 *   invert_variances  CodebookTrain::invertVariance (cT:218-223)
 *   split             DistribTrain::split (dT:92-109) -> CodebookTrain::split / _split (cT:122-198): the new Gaussian is appended to the codebook;
 *                     DSR_E_PARAMETER when maxCount < minCount, DSR_E_DIMENSION at 256 Gaussians; that codebook's and distribution's accumulators
 *                     start again at zero with the new size; *refX = the Gaussian that was split */
dsr_status dsr_train_update(dsr_train*, int what, int nParts, int part);
dsr_status dsr_train_update_mmi(dsr_train*, int what, double E, int merialdo, int nParts, int part);
dsr_status dsr_train_floor_variances(dsr_train*, int nParts, int part, unsigned* total, unsigned* floored);
dsr_status dsr_train_fix_gconsts(dsr_train*, int nParts, int part);
dsr_status dsr_train_invert_variances(dsr_train*, int nParts, int part);
dsr_status dsr_train_split(dsr_train*, int distX, float minCount, float splitFactor, unsigned* refX);
/* the model's parameters as the updates left them (host copies; any pointer may be NULL): refN [K], mean, cv [G][dimN], det, val, count [G] */
dsr_status dsr_gmm_get_params(const dsr_gmm*, int32_t* refN, float* mean, float* cv, float* det, float* val, float* count);
/* milliseconds of the two kernels of the last dsr_train_accumulate (posterior, contraction + reduction); 0 until timing is switched on */
dsr_status dsr_train_set_timing(dsr_train*, int on);
dsr_status dsr_train_kernel_ms(const dsr_train*, float ms[2]);

/* =====================================================================================
 * 10. MLLR speaker adaptation: regression classes, parameter trees, estimation, mean transforms
 *    Replaces the MLLR branch of asr/adapt/transform.{h,cc} ("tr") and asr/train/estimateAdapt.{h,cc} ("eA").  The all-pass transforms
 *    are section 13 (BLT and SLAPT with one estimated parameter; RAPT with more parameters and the multi-parameter Newton search are not
 *    implemented), STC and LDA section 12, the ML slice of asr/sat sections 14 and 14b.
 * ===================================================================================== */
/* The regression-class table of a model: CodebookBasic::_regClass (asr/gaussian/codebookBasic.cc:179-187).  dsr_gmm_load keeps the FIRST class
 * of each Gaussian of a codebook file whose regClassPresent is set (:286-297) -- GaussDensity::regClass() (codebookBasic.h:275-280) -- and
 * dsr_gmm_save writes the table as CodebookBasic::save does (:352-405), one class per Gaussian; a model without a table is saved as before.
 *   set_reg_class_all   CodebookSetBasic::setRegClasses(c) (:213-223, 1002-1006)
 *   set_reg_classes     one class per Gaussian [G], codebook after codebook
 *   get_reg_classes     the classes (0 where there is none) and whether the model has a table; either pointer may be NULL */
dsr_status dsr_gmm_set_reg_class_all(dsr_gmm*, unsigned c);
dsr_status dsr_gmm_set_reg_classes(dsr_gmm*, const uint16_t* perGaussian);
dsr_status dsr_gmm_get_reg_classes(const dsr_gmm*, uint16_t* perGaussian, int* present);
int dsr_gmm_num_gaussians(const dsr_gmm*);

/* ParamTree of MLLRParam (tr:520-552, 789-950; the text file of tr:203-407, 576-607).  Host only: needs no device.
 *   create      ParamTree(fileName): "" or NULL is an empty tree
 *   read        clear, then one parameter per <AdaptType> ... <EndClass> block; DSR_E_TYPE for a file of another adaptation type,
 *               DSR_E_PARAMETER for RAPT / SLAPT symbols or a second type inside a class, DSR_E_CONSISTENCY for a file without parameters
 *   write       the classes in index order, class 0 written as 1, numbers with " %g"
 *   type        0 unspecified, 3 MLLR (AdaptationType)
 *   find        mllr = 0: ParamTree::find (tr:835-860), 1: findMLLR (tr:898-925); with useAncestor a missing class becomes a copy of its
 *               nearest ancestor (findMLLR: an empty parameter when there is none); DSR_E_INDEX otherwise and for class 0; *size = the order
 *   get / set   W [size][size + 1], the last column the bias (MLLRParam::operator=(gsl_matrix*), tr:622-650); set goes through findMLLR
 *   indices     the classes in order (at most cap are written); returns their number */
typedef struct dsr_param_tree dsr_param_tree;
dsr_status dsr_param_tree_create(const char* fileName, dsr_param_tree** out);
void dsr_param_tree_destroy(dsr_param_tree*);
dsr_status dsr_param_tree_clear(dsr_param_tree*);
dsr_status dsr_param_tree_read(dsr_param_tree*, const char* fileName);
dsr_status dsr_param_tree_write(const dsr_param_tree*, const char* fileName);
dsr_status dsr_param_tree_copy(dsr_param_tree* dst, const dsr_param_tree* src);
int dsr_param_tree_type(const dsr_param_tree*);
int dsr_param_tree_has_index(const dsr_param_tree*, unsigned rc);
int dsr_param_tree_indices(const dsr_param_tree*, unsigned* indices, int cap);
dsr_status dsr_param_tree_find(dsr_param_tree*, unsigned rc, int useAncestor, int mllr, int* size);
dsr_status dsr_param_tree_get(const dsr_param_tree*, unsigned rc, double* W);
dsr_status dsr_param_tree_set(dsr_param_tree*, unsigned rc, int D, const double* W);
/* isAncestor (tr:133-145); DSR_E_INDEX when either index is 0 */
dsr_status dsr_is_ancestor(unsigned ancestor, unsigned child, int* result);

/* MLLR for S speakers at once (csrc/k_mllr.hip).  The handle copies the model's means (CodebookAdapt::_origRV: estimation and the transforms
 * always read these, codebookAdapt.h:99-104), inverse variances and regression classes when it is made; dimN <= 80.
 *   set_stats          count - denCount (postProb(), codebookTrain.h:142-144) and sumO of a trainer into slot s, device to device
 *   set_stats_arrays   the same from host arrays c [G], sumO [G][dimN]
 *   estimate           EstimatorTreeMLLR (eA:3143-3165) + estimateAdaptationParameters (eA:3064-3078) for every slot: the statistics
 *                      G_i = sum_g c iv_gi xi xi^T, z_i = sum_g sumO_gi iv_gi xi (xi = (mean, 1); _calcGi / _calcZ eA:2101-2153) of every node by an
 *                      fp64 MFMA contraction summed in a fixed order (they differ from the reference's sums by its float roundings of the terms
 *                      and by fp64 reordering; Gaussians whose count rounds to float 0 are skipped as there); LeafIterator::estimate's back-off
 *                      (eA:3105-3133) on the host; w_i = pinv(G_i) z_i with singular values below 1e-7 of the largest dropped (eA:2156-2180) by
 *                      a Jacobi eigen-decomposition.  Each slot's tree is replaced by the result.  DSR_E_INDEX for a Gaussian of class 0
 *                      (_setNode, tr:2019-2023); DSR_E_CONSISTENCY when some slot's statistics are not finite or did not converge: those
 *                      slots keep their trees (dsr_mllr_speaker_status), the others are done.
 *   get_plan           the steps of the last estimate, [n][4] = speaker, node, leaf, copy (1: copied from the nearest ancestor)
 *   get_nodes          the nodes of the regression tree in order and whether each is a leaf
 *   get_stats          G_i [dimN + 1][dimN + 1] and z_i [dimN + 1] of the last estimate;  ttl_frames  EstimatorAdapt::ttlFrames (eA:1565-1572)
 *   tree               the slot's parameter tree (owned by the handle)
 *   adapt              TransformerTree::transform (tr:2149-2163) of slot s into `target` (a model of the same shape): every Gaussian takes the
 *                      transform of node(regClass, useAncestor) -- DSR_E_KEY without one (tr:2030-2049) -- computed as MLLRTransformer::
 *                      transform does (tr:1770-1785: a float that starts at the bias and is rounded after every term); the model is re-uploaded
 *   adapt_all          the same for every slot into means_dev [S][G][dimN] (device)
 *   reset_mean         CodebookAdapt::resetMean: the original means back into `target` */
typedef struct dsr_mllr dsr_mllr;
dsr_status dsr_mllr_create(const dsr_gmm*, int S, dsr_mllr** out);
void dsr_mllr_destroy(dsr_mllr*);
int dsr_mllr_num_speakers(const dsr_mllr*);
dsr_status dsr_mllr_set_stats(dsr_mllr*, int s, dsr_train*);
dsr_status dsr_mllr_set_stats_arrays(dsr_mllr*, int s, const double* c, const double* sumO);
dsr_status dsr_mllr_estimate(dsr_mllr*, double threshold, void* stream);
int dsr_mllr_speaker_status(const dsr_mllr*, int s);
dsr_status dsr_mllr_get_plan(const dsr_mllr*, int* n, int32_t* steps);
dsr_status dsr_mllr_get_nodes(const dsr_mllr*, int* n, uint32_t* nodes, int32_t* isLeaf);
dsr_status dsr_mllr_get_stats(dsr_mllr*, int s, unsigned node, int row, double* G, double* z);
dsr_status dsr_mllr_ttl_frames(const dsr_mllr*, int s, unsigned node, double* ttl);
dsr_param_tree* dsr_mllr_tree(dsr_mllr*, int s);
dsr_status dsr_mllr_get_transform(dsr_mllr*, int s, unsigned rc, double* W);
dsr_status dsr_mllr_write(dsr_mllr*, int s, const char* fileName);
dsr_status dsr_mllr_read(dsr_mllr*, int s, const char* fileName);
dsr_status dsr_mllr_adapt(dsr_mllr*, int s, dsr_gmm* target);
dsr_status dsr_mllr_adapt_all(dsr_mllr*, float* means_dev, void* stream);
dsr_status dsr_mllr_reset_mean(dsr_mllr*, dsr_gmm* target);
/* milliseconds of the last statistics + reduction, solve and transform kernels; 0 until timing is switched on */
dsr_status dsr_mllr_set_timing(dsr_mllr*, int on);
dsr_status dsr_mllr_kernel_ms(const dsr_mllr*, float ms[3]);

/* =====================================================================================
 * 11. Feature-space adaptation (constrained MLLR)
 *    Replaces FeatureSpaceAdaptationFeature (asr/train/fsa.{h,cc}, "fsa"; train.i:531-590): one affine transform W = (b | A) [dimN][dimN + 1] of
 *    the features per transformation slot, estimated from statistics gathered with the nearest Gaussian of each (frame, distribution) item.
 *    One item is _accuOne(dsX, frameX, accuX, gamma) (fsa:187-245): distributions not switched on by add / add_all are ignored before anything
 *    is counted (nothing is on at first); count++ and the float sum beta += gamma in item order; g = the nearest Gaussian of the codebook under
 *    the SCORING frame (the one-hot addCount of CodebookBasic::_scoreOpt, codebookBasic.cc:431-554: the argmin of scoring mode 0, found with the
 *    model's scoring tables); with xi = (1, x) of the SOURCE frame (the untransformed _src, fsa:195)
 *        z[i][.] += (gamma float(mean_gi iv_gi)) xi        G_i[j][k] += (gamma iv_gi) xi_j xi_k   for k <= j
 *    in fp64.  Only the lower triangle and column 0 of G_i are written (fsa:235-241).  The sums over the items of a call are an fp64 MFMA
 *    contraction in a fixed order (no atomics: the same call twice gives the same bits); they differ from the reference's sequential sums by
 *    fp64 reordering and by its roundings of c xi_j and (c xi_j) xi_k, which the contraction skips.  The means and inverse variances of the
 *    statistics are copied when the handle is made; the model must outlive the handle.  dimN <= 80.  _dimN, in the reference the feature
 *    length of the codebook with the most Gaussians (fsa:48-54), is the model's dimN: the codebooks of a dsr_gmm share it, so the
 *    jdimension_error of add (fsa:165-167) cannot arise.  The constructor's use of _maxAccu before it is set (fsa:36) is not reproduced.
 *   create             FeatureSpaceAdaptationFeature(src, maxAccu, maxTran) + _initialize (fsa:32-112): zeroed accumulators, identity transforms
 *   add / add_all      fsa:159-176; DSR_E_INDEX for a distribution outside the set
 *   set_top_n          setTopN: kept for the interface; the entries after the first are ties at addCount 0 and add c = 0 terms (fsa:203-244).
 *                      DSR_E_INDEX for topN beyond refN of the largest codebook, where the reference reads past its arrays
 *   accumulate         M items over xScore_dev, xSrc_dev [N][dimN] fp32 (they may be the same array) with host arrays frame, dist, gamma, accu [M];
 *                      accepted [nAccu] or NULL: the items each accumulator took; nearest [M] or NULL: the Gaussian (inside its codebook) each item
 *                      chose, -1 for a distribution that is not switched on.  DSR_E_INDEX: a frame, distribution or accumulator out of range
 *   accumulate_path    accumulate(path, accuX, factor) (fsa:282-297): distIds [pathLen], a negative id is a name that was not found and does NOT
 *                      advance the frame index, as there; *framesN = the frames the reference reports ("Accumulated n frames.")
 *   accumulate_lattice accumulateLattice(lat, accuX, factor) (fsa:299-321) with the lattice's current gammas, links in the order of
 *                      dsr_train_accumulate_lattice: input 0 and gamma > 10 are skipped, postProb = float(factor exp(-gamma)), and -- the loop
 *                      increments frameX in its header and again in the call (fsa:317-318) -- every SECOND frame start, start + 2, ... of a link
 *   zero / scale / add_accu   zeroAccu, scaleAccu, addAccu (fsa:435-465, 637-650) as written
 *   get_accu / set_accu       count, beta, z [dimN][dimN + 1], G [dimN][dimN + 1][dimN + 1] with the triangle as the reference holds it
 *   save_accu / load_accu     magic "SAS", big-endian floats (fsa:505-583): count and every element rounded to float, the upper triangle as it
 *                      stands; loading ADDS factor x the file.  DSR_E_CONSISTENCY without the magic, DSR_E_DIMENSION for another dimN
 *   estimate           estimate(iterN, accuX, tranX) (fsa:363-433) for n (accumulator, transformation) pairs at once, each from its CURRENT
 *                      transform: G_i^+ with singular values below 1e-7 of the largest dropped (a Jacobi eigen-decomposition), then iterN sweeps of
 *                      row updates with p = det A . A^-1[:, i] (the reference takes |det| from an SVD of A per row; the sign cancels in w_i).
 *                      DSR_E_PARAMETER when a transformation is named twice.  A pair whose statistics or result are not finite (fewer than
 *                      dimN + 1 frames: the reference stores NaN), whose decomposition does not converge or whose ||A||_F ||A^-1||_F reaches 1e7
 *                      (the reference's 1e-7 rule in _calcCofactor could then have dropped a singular value of A) keeps its transform and is
 *                      flagged (transform_status); the others are done and the call returns DSR_E_CONSISTENCY, as dsr_mllr_estimate does
 *   get / set_transform, clear (fsa:467-481), compare (compareTransform, fsa:483-503: squares over columns 0 .. dimN - 1 as written, float)
 *   save / load        magic "SAW" (fsa:585-635); DSR_E_IO without the magic, DSR_E_DIMENSION for another dimN
 *   apply              next (fsa:247-280) for N frames: out = float(shift w[d][0] + sum_i w[d][i + 1] x_i), a double sum with i ascending; for
 *                      shift == -1 float(w[d][0] + x_d).  tranOfRow_dev int32 [N] (device) names each row's transformation -- what a batch of
 *                      mixed speakers needs --, NULL is transformation 0; a row whose index is out of range becomes NaN
 *   kernel_ms          milliseconds of the last nearest-Gaussian, statistics + reduction, eigen-decomposition, row-update and apply kernels
 * ===================================================================================== */
typedef struct dsr_fsa dsr_fsa;
dsr_status dsr_fsa_create(dsr_gmm*, int nAccu, int nTran, dsr_fsa** out);
void dsr_fsa_destroy(dsr_fsa*);
int dsr_fsa_dim(const dsr_fsa*);
int dsr_fsa_num_accus(const dsr_fsa*);
int dsr_fsa_num_transforms(const dsr_fsa*);
dsr_status dsr_fsa_add(dsr_fsa*, int dsX);
dsr_status dsr_fsa_add_all(dsr_fsa*);
dsr_status dsr_fsa_set_top_n(dsr_fsa*, unsigned topN);
unsigned dsr_fsa_top_n(const dsr_fsa*);
dsr_status dsr_fsa_set_shift(dsr_fsa*, float shift);
float dsr_fsa_shift(const dsr_fsa*);
dsr_status dsr_fsa_count(const dsr_fsa*, int accuX, double* count);
dsr_status dsr_fsa_accumulate(dsr_fsa*, const float* xScore_dev, const float* xSrc_dev, int64_t N, const int32_t* frame, const int32_t* dist,
                              const float* gamma, const int32_t* accu, int64_t M, int64_t* accepted, int32_t* nearest, void* stream);
dsr_status dsr_fsa_accumulate_path(dsr_fsa*, const float* xScore_dev, const float* xSrc_dev, int64_t T, const int32_t* distIds, int64_t pathLen,
                                   int accuX, float factor, unsigned* framesN, void* stream);
dsr_status dsr_fsa_accumulate_lattice(dsr_fsa*, dsr_lattice*, const float* xScore_dev, const float* xSrc_dev, int64_t T, int accuX, float factor,
                                      unsigned* linksN, void* stream);
/* for callers without a HIP binding of their own (host/dsr_streams.hpp): N frames of dimN floats each from host memory into buffers the handle
 * owns; the device pointers stay valid until the next upload or the handle's end */
dsr_status dsr_fsa_upload_features(dsr_fsa*, const float* xScore_host, const float* xSrc_host, int64_t N, const float** xScore_dev, const float** xSrc_dev);
dsr_status dsr_fsa_zero(dsr_fsa*, int accuX);
dsr_status dsr_fsa_scale(dsr_fsa*, float scale, int accuX);
dsr_status dsr_fsa_add_accu(dsr_fsa*, int accuX, int accuY, float factor);
dsr_status dsr_fsa_get_accu(const dsr_fsa*, int accuX, double* count, float* beta, double* z, double* G);
dsr_status dsr_fsa_set_accu(dsr_fsa*, int accuX, const double* count, const float* beta, const double* z, const double* G);
dsr_status dsr_fsa_save_accu(const dsr_fsa*, const char* fileName, int accuX);
dsr_status dsr_fsa_load_accu(dsr_fsa*, const char* fileName, int accuX, float factor);
dsr_status dsr_fsa_estimate(dsr_fsa*, int iterN, const int32_t* accuX, const int32_t* tranX, int n, void* stream);
int dsr_fsa_transform_status(const dsr_fsa*, int tranX);
dsr_status dsr_fsa_get_transform(const dsr_fsa*, int tranX, double* W);
dsr_status dsr_fsa_set_transform(dsr_fsa*, int tranX, const double* W);
dsr_status dsr_fsa_clear(dsr_fsa*, int tranX);
dsr_status dsr_fsa_compare(const dsr_fsa*, int tranX, int tranY, float* sumOfSquares);
dsr_status dsr_fsa_save(const dsr_fsa*, const char* fileName, int tranX);
dsr_status dsr_fsa_load(dsr_fsa*, const char* fileName, int tranX);
dsr_status dsr_fsa_apply(dsr_fsa*, const float* x_dev, int64_t N, const int32_t* tranOfRow_dev, float shift, float* out_dev, void* stream);
dsr_status dsr_fsa_set_timing(dsr_fsa*, int on);
dsr_status dsr_fsa_kernel_ms(const dsr_fsa*, float ms[5]);
/* The stream operator (a VectorFloatFeatureStream, fsa.h): src under transformation 0 and the handle's shift, frames kept on the device, so
 * dsr_distribset_create(gmm, stream, ...) + dsr_decoder_decode_stream decode adapted frames without a host round trip.
 *   distrib_set   distribSet(dss): makes the adaptation handle (zeroed accumulators, identity transforms) for the model
 *   handle        the operator's dsr_fsa, owned by the stream; NULL before distrib_set
 * next() before distrib_set is DSR_E_CONSISTENCY (fsa:251-252), an out-of-order frameX DSR_E_INDEX (fsa:254-255).  A new transform or shift
 * shows after the next reset(). */
dsr_status dsr_fsa_feature_create(dsr_stream* src, int maxAccu, int maxTran, const char* name, dsr_stream** out);
dsr_status dsr_fsa_feature_distrib_set(dsr_stream*, dsr_gmm*);
dsr_fsa* dsr_fsa_feature_handle(dsr_stream*);

/* ---------------------------------------------------------------------------------------------------------------------------------------
 * 12. Semi-tied covariance (STC) and LDA transforms: estimation and application (csrc/k_stc.hip, csrc/stc.cpp, csrc/stc_rows.h)
 *
 *    Replaces STCTransformer / LDATransformer (asr/adapt/transform.cc:1788-1984, "tr") and STCEstimator / LDAEstimator
 *    (asr/train/estimateAdapt.cc:2203-3036, "eA"; train.i:390-500) for models of one sub-feature (nSubFeat = 1, subFeatLen = dimN <= 64).
 *    A handle holds nEst estimators over one model; one item is (frame, distribution, factor, estimator).  The Gaussian of an item is the
 *    one-hot addCount of CodebookBasic::_scoreOpt under the SCORING frame, found with scoring mode 0's arithmetic; the statistics are made
 *    from the SOURCE frame.  The sums over the items of a call are fp64 MFMA contractions cut into fixed chunks and reduced in a fixed order
 *    (no floating-point atomics).  The means and inverse variances the statistics use are copied when the handle is created (as dsr_fsa does),
 *    while the nearest Gaussian is found with the model's live tables: a handle is made after the model's last update; the model must outlive
 *    it.  The host adds the sums to accumulators it holds as the reference does: the lower triangle is written, and
 *    copyUpperTriangle runs on every read through the reference's accessors (estimateAdapt.h:688-689, 813-815) -- get_accu with
 *    throughAccessor != 0, save_accu and estimate.
 *
 *  STC
 *   create             STCEstimator(src, pt, dss, idx, bt, cascade, mmiEstimation, ...) (eA:2205-2235): zeroed accumulators, identity matrices
 *   create_transformer STCTransformer(src, sbFtSz, nSubFt, nm) (tr:1790-1796): one matrix and no statistics: accumulate, estimate and every
 *                      accumulator entry (increment, zero, get / set_accu, save / load_accu, aux) return DSR_E_CONSISTENCY; the same for LDA
 *   accumulate         accumulateW1 / accumulateW2 (eA:2569-2651) over M items: o = float(x - mu_g), wgt_d = float(iv_gd float(addCount factor)),
 *                      sumOsq[d][i][j] += (wgt_d o_i) o_j for j <= i; _count / _denCount per item as eA:2581-2584; for factor <= 0
 *                      regSq[d] += iv_gd sum_col float(c / iv_g,col) a_col a_col^T with a_col the columns of _stcInv, summed as
 *                      R[d][col] = sum_n iv[n,d] float(c_n / iv[n,col]) on the device and R[d][col] a_col a_col^T once on the host: the float
 *                      roundings stand where the reference has them, only the order of the fp64 sum differs.  With cascade the source frame
 *                      is first put under the estimator's current matrix (eA:2276-2278).  nearest [M] / score [M] (or NULL): the Gaussian
 *                      inside its codebook and the distribution's mode 0 score of every item.
 *   accumulate_path    accumulate(path, factor) (eA:2265-2294): distIds [pathLen], one distribution per frame from frame 0, then increment
 *                      (eA:2284-2287).  A negative id is DSR_E_INDEX (DistribSet::find throws there).
 *   increment, zero    Accu::increment (estimateAdapt.h:681), Accu::zero (eA:2511-2519)
 *   get / set_accu     _count, _denCount, _totalPr, _totalT, sumOsq [dimN][dimN][dimN], regSq likewise
 *   save / load_accu   Accu::save / load (eA:2521-2566): big-endian ints and floats (counts and totalPr rounded to float), matrices raw native
 *                      doubles as gsl_matrix_fwrite writes them; loading ADDS; DSR_E_DIMENSION for another dimN or nSubFeat != 1
 *   estimate           estimate(rc, minE, multE) (eA:2296-2316) for n estimators at once: makePosDef (eA:2689-2711), the inverses of
 *                      sumOsq[d] + E regSq[d] (eA:2400-2410) and MaxItns = 10 sweeps of row updates (eA:2416-2448) on the device.  Only the
 *                      sign of det A is carried.  With cascade the new matrix left-multiplies the old (eA:2298-2307); _stcInv is refreshed.
 *                      An estimator whose statistics are not finite, cannot be made positive definite, whose inner product is <= 0 (the
 *                      reference's jnumeric_error, eA:2434-2435) or whose matrix leaves ||A||_F ||A^-1||_F < 1e7 keeps its matrix; the others
 *                      of the call are done and the call returns DSR_E_CONSISTENCY.  status: 0 or DSR_E_CONSISTENCY of the last estimate.
 *   E                  Accu::E() of the last estimate
 *   aux                2 gamma log |det A| - sum_d a_d (sumOsq[d] + E regSq[d]) a_d^T, gamma = count or denCount E: the function the row
 *                      update maximises.  NOT calcAuxFunc's printed value (eA:2665-2686), whose E term stands outside the product.
 *                      A == NULL: the estimator's matrix.
 *   get / set_transform  matrix() and _stcInv as doubles; set refreshes _stcInv (DSR_E_CONSISTENCY for a singular matrix)
 *   trans_matrix       transMatrix() (eA:2318-2325): the float copy
 *   save / load        STCTransformer::save / load (tr:1852-1864): raw doubles; load refreshes _stcInv as STCEstimator::load (eA:2348-2356)
 *   save_float         STCEstimator::save(fileName, trans) (eA:2327-2346): the float matrix, times trans [dimN][dimN] when given
 *   apply              _transform (tr:1866-1879): out = float(sum_j double(x_j) A[i][j]), j ascending, no bias
 *   kernel_ms          nearest, statistics + reduction, eigen-decompositions, rows, apply (after set_timing)
 *
 *  LDA
 *   create             LDAEstimator(src, pt, dss, globalCodebook, ...) (eA:2716-2735): global = a model whose codebook 0 is the global codebook.
 *                      The reference never zeroes its accumulators before use (eA:2877-2894); here they start from zero.
 *   create_transformer LDATransformer(src, sbFtSz, nSubFt, nm) (tr:1884-1897)
 *   accumulate         Accu::accumulate (eA:2989-3036): count = float(addCount factor); within += count oW oW^T, between += count oB oB^T,
 *                      mixture += count oM oM^T over j <= i with the float differences oW = x - mu_g, oB = mu_g - mu_0, oM = x - mu_0, mu_0
 *                      Gaussian 0 of the global codebook.  A codebook whose refN differs from the global codebook's is DSR_E_DIMENSION (eA:2995).
 *   accumulate_path    accumulate(path, factor) (eA:2761-2790) -> the summed score
 *   zero, get / set_accu, save / load_accu   eA:2908-2980: matrices raw doubles, the count last and as a float
 *   estimate           estimate(rc) (eA:2752-2836): scaleScatterMatrices divides the accumulators IN PLACE (a second estimate divides again),
 *                      then the simultaneous diagonalisation by two Jacobi eigen-decompositions on the device, n estimators a call
 *   eigenvalues        of `within` (as found) and of the whitened `between` (descending) of the last estimate
 *   get / set_transform, apply   the Din x Din matrix; apply writes the first outDim rows (tr:1948-1955)
 *   save / load        LDATransformer::save writes float32, load reads float64 (tr:1961-1984, the reference's own "HACK"): kept as they are
 */
typedef struct dsr_stc dsr_stc;
typedef struct dsr_lda dsr_lda;
dsr_status dsr_stc_create(dsr_gmm*, int nEst, int cascade, int mmiEstimation, dsr_stc** out);
dsr_status dsr_stc_create_transformer(int dimN, dsr_stc** out);
void dsr_stc_destroy(dsr_stc*);
int dsr_stc_dim(const dsr_stc*);
int dsr_stc_num_estimators(const dsr_stc*);
dsr_status dsr_stc_accumulate(dsr_stc*, const float* xScore_dev, const float* xSrc_dev, int64_t N, const int32_t* frame, const int32_t* dist,
                              const float* factor, const int32_t* est, int64_t M, int32_t* nearest, float* score, void* stream);
dsr_status dsr_stc_accumulate_path(dsr_stc*, const float* xScore_dev, const float* xSrc_dev, int64_t T, const int32_t* distIds, int64_t pathLen,
                                   int estX, float factor, unsigned* framesN, void* stream);
/* frames of a host program: copied to buffers the handle owns (valid until the next call) */
dsr_status dsr_stc_upload_features(dsr_stc*, const float* xScore_host, const float* xSrc_host, int64_t N, const float** xScore_dev, const float** xSrc_dev);
dsr_status dsr_stc_increment(dsr_stc*, int estX, double totalPr, unsigned totalT);
dsr_status dsr_stc_zero(dsr_stc*, int estX);
dsr_status dsr_stc_get_accu(dsr_stc*, int estX, int throughAccessor, double* count, double* denCount, double* totalPr, unsigned* totalT, double* sumOsq,
                            double* regSq);
dsr_status dsr_stc_set_accu(dsr_stc*, int estX, const double* count, const double* denCount, const double* totalPr, const unsigned* totalT,
                            const double* sumOsq, const double* regSq);
dsr_status dsr_stc_save_accu(dsr_stc*, const char* fileName, int estX);
dsr_status dsr_stc_load_accu(dsr_stc*, const char* fileName, int estX);
dsr_status dsr_stc_estimate(dsr_stc*, const int32_t* estX, int n, double minE, double multE, void* stream);
int dsr_stc_status(const dsr_stc*, int estX);
dsr_status dsr_stc_E(const dsr_stc*, int estX, double* E);
dsr_status dsr_stc_aux(const dsr_stc*, int estX, const double* A, double E, double* aux);
dsr_status dsr_stc_get_transform(const dsr_stc*, int estX, double* A, double* Ainv);
dsr_status dsr_stc_set_transform(dsr_stc*, int estX, const double* A);
dsr_status dsr_stc_trans_matrix(const dsr_stc*, int estX, float* out);
dsr_status dsr_stc_save(const dsr_stc*, const char* fileName, int estX);
dsr_status dsr_stc_load(dsr_stc*, const char* fileName, int estX);
dsr_status dsr_stc_save_float(const dsr_stc*, const char* fileName, int estX, const float* trans);
dsr_status dsr_stc_apply(dsr_stc*, const float* x_dev, int64_t N, int estX, float* out_dev, void* stream);
dsr_status dsr_stc_set_timing(dsr_stc*, int on);
dsr_status dsr_stc_kernel_ms(const dsr_stc*, float ms[5]);
dsr_status dsr_lda_create(dsr_gmm*, dsr_gmm* global, int nEst, dsr_lda** out);
dsr_status dsr_lda_create_transformer(int dimN, dsr_lda** out);
void dsr_lda_destroy(dsr_lda*);
int dsr_lda_dim(const dsr_lda*);
int dsr_lda_num_estimators(const dsr_lda*);
dsr_status dsr_lda_accumulate(dsr_lda*, const float* xScore_dev, const float* xSrc_dev, int64_t N, const int32_t* frame, const int32_t* dist,
                              const float* factor, const int32_t* est, int64_t M, int32_t* nearest, float* score, void* stream);
dsr_status dsr_lda_accumulate_path(dsr_lda*, const float* xScore_dev, const float* xSrc_dev, int64_t T, const int32_t* distIds, int64_t pathLen,
                                   int estX, float factor, double* score, void* stream);
dsr_status dsr_lda_upload_features(dsr_lda*, const float* xScore_host, const float* xSrc_host, int64_t N, const float** xScore_dev, const float** xSrc_dev);
dsr_status dsr_lda_zero(dsr_lda*, int estX);
dsr_status dsr_lda_get_accu(dsr_lda*, int estX, int throughAccessor, double* count, double* within, double* between, double* mixture);
dsr_status dsr_lda_set_accu(dsr_lda*, int estX, const double* count, const double* within, const double* between, const double* mixture);
dsr_status dsr_lda_save_accu(dsr_lda*, const char* fileName, int estX);
dsr_status dsr_lda_load_accu(dsr_lda*, const char* fileName, int estX);
dsr_status dsr_lda_estimate(dsr_lda*, const int32_t* estX, int n, void* stream);
int dsr_lda_status(const dsr_lda*, int estX);
dsr_status dsr_lda_eigenvalues(const dsr_lda*, int estX, double* withinEv, double* betweenEv);
dsr_status dsr_lda_get_transform(const dsr_lda*, int estX, double* L);
dsr_status dsr_lda_set_transform(dsr_lda*, int estX, const double* L);
dsr_status dsr_lda_save(const dsr_lda*, const char* fileName, int estX);
dsr_status dsr_lda_load(dsr_lda*, const char* fileName, int estX);
dsr_status dsr_lda_apply(dsr_lda*, const float* x_dev, int64_t N, int estX, int outDim, float* out_dev, void* stream);
dsr_status dsr_lda_set_timing(dsr_lda*, int on);
dsr_status dsr_lda_kernel_ms(const dsr_lda*, float ms[5]);
/* The stream operators (VectorFloatFeatureStreams): src under matrix 0 of the operator's handle -- for LDA its first outDim rows --, frames
 * kept on the device, so dsr_distribset_create(gmm, stream, ...) + dsr_decoder_decode_stream decode transformed frames without a host round
 * trip.  The handle is a bare transformer until distrib_set / codebooks names the model; it keeps its matrix then.  A new matrix shows after
 * the next reset(). */
dsr_status dsr_stc_feature_create(dsr_stream* src, int cascade, int mmiEstimation, const char* name, dsr_stream** out);
dsr_status dsr_stc_feature_distrib_set(dsr_stream*, dsr_gmm*);
dsr_stc* dsr_stc_feature_handle(dsr_stream*);
dsr_status dsr_lda_feature_create(dsr_stream* src, int outDim, const char* name, dsr_stream** out);
dsr_status dsr_lda_feature_codebooks(dsr_stream*, dsr_gmm*, dsr_gmm* global);
dsr_lda* dsr_lda_feature_handle(dsr_stream*);

/* ---------------------------------------------------------------------------------------------------------------------------------------
 * 13. All-pass transform (APT) speaker adaptation: the bilinear transform (BLT) and the sine-log all-pass transform (SLAPT)
 *     (csrc/apt_kernels.hip, csrc/apt.cpp)
 *
 *    Replaces LaurentSeries, APTParamBase / RAPTParam / SLAPTParam, ParamTree::findAPT, BLTTransformer and SLAPTTransformer
 *    (asr/adapt/transform.cc, "tr": 39-101, 410-551, 862-896, 1199-1430, 1636-1741) and BLTEstimatorAdapt, SLAPTEstimatorAdapt with one
 *    parameter, EstimatorBase::bracket / brentsMethod (asr/train/estimateAdapt.cc, "eA": 81-255, 821-830, 1544-1690, 1851-1929, 2026-2045).
 *    A cepstral mean of nSubFeat sub-features of subFeatLen (flat index isub subFeatLen + n) is mapped by one subFeatLen x subFeatLen
 *    matrix per regression class, read off the powers of a Laurent series Q(z) of 150 coefficients a side, plus an optional bias.
 *    Not implemented, and refused: RAPT with more than one parameter, estimation of more than one parameter (the Newton search with
 *    gradient and Hessian matrices), an ldaFile, extended means (orgSubFeatLen != subFeatLen).
 *
 *  Parameters (host only: needs no device).  A dsr_apt_params is the ParamTree of one speaker, of RAPTParam or of SLAPTParam; dsr_param_tree
 *  keeps refusing these files.  type: 0 unspecified, 1 RAPT, 2 SLAPT (AdaptationType + 1).
 *   create / read   one parameter per <AdaptType> ... <EndClass> block (tr:339-407, 430-441, 927-950), numbers read with fscanf; DSR_E_TYPE for
 *                   a file that does not start with <AdaptType>, DSR_E_PARAMETER for an MLLR block, for the other type's symbol inside a
 *                   class or a second type inside a class (the jparameter_errors of _readParams), DSR_E_CONSISTENCY for blocks of both types
 *                   or a file without parameters.  "" or NULL is an empty store
 *   write           the classes in index order, class 0 written as 1, numbers with " %g"; RAPT writes fabs of its even-indexed parameters
 *                   from index 2 on (tr:490-501)
 *   find            ParamTree::findAPT (tr:862-896): DSR_E_CONSISTENCY for a store of the other type, DSR_E_INDEX for class 0 or a missing
 *                   class without useAncestor; with it a missing class becomes a copy of its nearest ancestor (an empty one without)
 *   get / set       _conf as doubles and the bias as floats; set goes through findAPT; sizes come from find
 *   line_search     EstimatorBase::bracket + brentsMethod (eA:109-240) replayed on the n values lhood[] = calcLogLhood of the points it asked
 *                   for so far; kind 1: b = 0, a = 0.1, range +-0.899 (BLT, eA:252-255, 1659-1665), 2: a = -0.05, b = 0, range +-100 (SLAPT,
 *                   eA:821-826, 1544-1548).  *state = 0: *point is the next point to evaluate; 1: done, *point = alpha / xmin; 2: bracket met
 *                   a NaN (eA:122-130) or Brent's method ran 100 iterations.  points [*nPoints] (or NULL): the points evaluated so far */
typedef struct dsr_apt_params dsr_apt_params;
dsr_status dsr_apt_params_create(const char* fileName, dsr_apt_params** out);
void dsr_apt_params_destroy(dsr_apt_params*);
dsr_status dsr_apt_params_clear(dsr_apt_params*);
dsr_status dsr_apt_params_read(dsr_apt_params*, const char* fileName);
dsr_status dsr_apt_params_write(const dsr_apt_params*, const char* fileName);
dsr_status dsr_apt_params_copy(dsr_apt_params* dst, const dsr_apt_params* src);
int dsr_apt_params_type(const dsr_apt_params*);
int dsr_apt_params_indices(const dsr_apt_params*, unsigned* indices, int cap);
dsr_status dsr_apt_params_find(dsr_apt_params*, unsigned rc, int type, int useAncestor, int* nConf, int* nBias);
dsr_status dsr_apt_params_get(const dsr_apt_params*, unsigned rc, double* conf, float* bias);
dsr_status dsr_apt_params_set(dsr_apt_params*, unsigned rc, int type, int nConf, const double* conf, int nBias, const float* bias);
dsr_status dsr_apt_line_search(int kind, const double* lhood, int n, int* state, double* point, int* nPoints, double* points);

/* APT for S speakers at once.  The handle copies the model's means (CodebookAdapt::_origRV), inverse variances and regression classes.
 *   create             kind 1 (BLT: a RAPTParam of one parameter) or 2 (SLAPT); subFeatLen nSubFeat == dimN, nSubFeat <= 3, subFeatLen <= 48;
 *                      biasType 0 NONE, 1 CepstraOnly (subFeatLen entries), 2 AllComponents (dimN entries) (eA:49-63, 1553-1563)
 *   set_param_n        the number of parameters to estimate: DSR_E_PARAMETER unless 1
 *   set_stats(_arrays) as dsr_mllr_set_stats(_arrays)
 *   set / get_params   (conf [nConf], bias [nBias]) of slot s and class rc; get with NULL arrays returns the sizes
 *   estimate           for every slot LeafIterator::estimate (eA:3105-3133) over the regression tree: a leaf whose ttlFrames (a double sum in
 *                      model order) does not exceed `threshold` backs off to its nearest ancestor that does (node 1 at last); that node's
 *                      Gaussians (class equal to it or below it) are searched and the result is stored under the LEAF's class.  There is no
 *                      copying for a tree that is not MLLR, and a slot's other classes stay.  The search does not start from what is
 *                      stored, so each (slot, node) is searched once.  The line searches run on the host; every round evaluates the trial
 *                      points of all running searches in one launch each of k_apt_matrix and k_apt_lhood.  calcLogLhood (eA:1638-1657,
 *                      1851-1884) is the reference's except that the bias sums of _calcBias and the sum over the Gaussians of _calcMixLhood
 *                      are fp64 sums in a fixed order (the same call twice gives the same bits).  Stored: _conf = alpha (BLT) or xmin
 *                      (SLAPT); the bias of _calcBias under the matrix at alpha (BLT, eA:1667-1668) or under the matrix of the LAST
 *                      EVALUATED trial point (SLAPT, eA:1926: the series still in _laurentCoeffs), not xmin.  DSR_E_INDEX for a Gaussian of
 *                      class 0; DSR_E_CONSISTENCY for a slot that holds parameters of the other type or (BLT) more than one; DSR_E_DIMENSION
 *                      (SLAPT) for a stored bias of another size: nothing is estimated then.  A slot whose search met a NaN in bracket or
 *                      ran 100 Brent iterations keeps its parameters and is flagged (speaker_status); the others are done and the call
 *                      returns DSR_E_CONSISTENCY
 *   get_plan           [n][3] = speaker, node, leaf;  get_nodes, ttl_frames as dsr_mllr;  rounds  the launches of each kernel in the last estimate
 *   get_trace          the (point, logLhood) pairs, in order, that the last estimate evaluated for (slot, node), and the bias [n][bias size] of
 *                      _calcBias at each; any array may be NULL.  DSR_E_KEY for a pair that was not searched
 *   get_matrix         the subFeatLen x subFeatLen matrix of the parameters node(rc, useAncestor) of slot s holds (_calcTransMatrix,
 *                      tr:1212-1242, of bilinear tr:1404-1414 or _calcSequence tr:1716-1741; any number <= 32 of SLAPT parameters): bit for
 *                      bit the reference's arithmetic.  DSR_E_PARAMETER for |mu| >= 1, RAPT parameters other than one, no SLAPT parameters
 *   adapt              TransformerTree::transform (tr:2149-2163) of slot s into `target`: every Gaussian takes node(regClass, useAncestor) --
 *                      DSR_E_KEY without one -- and component (isub, n) becomes float(sum_m A[n][m] double(mean(isub, m))), m ascending, plus
 *                      the float bias where it has an entry (tr:1295-1337).  A bias of another size than 0, subFeatLen or dimN is
 *                      DSR_E_CONSISTENCY.  adapt_all: every slot into means_dev [S][G][dimN] (device);  reset_mean: the original means back
 *   kernel_ms          milliseconds of k_apt_matrix and k_apt_lhood summed over the rounds of the last estimate, and of the last k_apt_apply */
typedef struct dsr_apt dsr_apt;
dsr_status dsr_apt_create(const dsr_gmm*, int S, int kind, int subFeatLen, int nSubFeat, int biasType, dsr_apt** out);
void dsr_apt_destroy(dsr_apt*);
int dsr_apt_num_speakers(const dsr_apt*);
dsr_status dsr_apt_set_param_n(dsr_apt*, int paramN);
dsr_status dsr_apt_set_stats(dsr_apt*, int s, dsr_train*);
dsr_status dsr_apt_set_stats_arrays(dsr_apt*, int s, const double* c, const double* sumO);
dsr_apt_params* dsr_apt_store(dsr_apt*, int s);
dsr_status dsr_apt_set_params(dsr_apt*, int s, unsigned rc, int nConf, const double* conf, int nBias, const float* bias);
dsr_status dsr_apt_get_params(const dsr_apt*, int s, unsigned rc, int* nConf, double* conf, int* nBias, float* bias);
dsr_status dsr_apt_estimate(dsr_apt*, double threshold, void* stream);
int dsr_apt_speaker_status(const dsr_apt*, int s);
int dsr_apt_rounds(const dsr_apt*);
dsr_status dsr_apt_get_plan(const dsr_apt*, int* n, int32_t* steps);
dsr_status dsr_apt_get_nodes(const dsr_apt*, int* n, uint32_t* nodes, int32_t* isLeaf);
dsr_status dsr_apt_ttl_frames(const dsr_apt*, int s, unsigned node, double* ttl);
dsr_status dsr_apt_get_trace(const dsr_apt*, int s, unsigned node, int* n, double* points, double* lhood, float* bias);
dsr_status dsr_apt_get_matrix(dsr_apt*, int s, unsigned rc, double* A);
dsr_status dsr_apt_write(dsr_apt*, int s, const char* fileName);
dsr_status dsr_apt_read(dsr_apt*, int s, const char* fileName);
dsr_status dsr_apt_adapt(dsr_apt*, int s, dsr_gmm* target);
dsr_status dsr_apt_adapt_all(dsr_apt*, float* means_dev, void* stream);
dsr_status dsr_apt_reset_mean(dsr_apt*, dsr_gmm* target);
dsr_status dsr_apt_set_timing(dsr_apt*, int on);
dsr_status dsr_apt_kernel_ms(const dsr_apt*, float ms[3]);
/* A transformer on its own (BLTTransformer(par, sbFtSz, nSubFt) / SLAPTTransformer(par, ...), tr:1379-1392, 1678-1698): the matrix of the
 * parameters (A [subFeatLen][subFeatLen], or NULL) and transform(from, to) (tr:1295-1337) of N host rows [subFeatLen nSubFeat] into out, both
 * computed on the device by k_apt_matrix and k_apt_apply.  The errors of get_matrix and adapt */
dsr_status dsr_apt_transform_rows(int kind, int subFeatLen, int nSubFeat, int nConf, const double* conf, int nBias, const float* bias,
                                  const float* rows, int N, double* A, float* out);

/* ---------------------------------------------------------------------------------------------------------------------------------------
 * 14. Speaker-adaptive training (ML-SAT): the canonical means and variances given every speaker's transform and statistics
 *     (csrc/sat_kernels.hip, csrc/sat.cpp)
 *
 *    Replaces SATMean (asr/sat/sat.cc, "sat": 54-342), SATVariance (sat:686-760), SATBase::MeanAcc (sat:999-1025), SATBase::VarianceAcc
 *    (sat:1194-1246), SATBase and SAT<Type> = MeanSAT / VarianceSAT (sat:1763-1855, sat.h:736-800), TransformerTreeList::getTree
 *    (sat:1884-1896) and SpeakerList (asr/adapt/transform.cc, "tr": 1989-1998) for the diagonal 1:1 models of dsr_gmm with
 *    orgFeatLen == featLen, under MLLR transforms (one block dimN x dimN, tr:1746-1785) and BLT / SLAPT transforms (nSubFeat blocks of
 *    subFeatLen^2 holding the same matrix, the bias as the block offsets, tr:1339-1363).
 *    MDLSATMean (a likelihood threshold), FastSAT / FastAcc and the CodebookFastSAT accumulators are section 14b (dsr_fsat_*); dsr_sat_check
 *    and the two classes of this section keep refusing them.  Not implemented, here or there: RegClassAcc / MMIRegClassAcc, MMIAcc /
 *    FastMMISAT, SATMeanFullCovar, cluster.cc, extended means, an ldaFile; STC / LDA blocks in a speaker file are refused by the parameter
 *    readers.
 *
 *   check              the options of SAT<Type>(cbs, meanLen, lhoodThreshhold, massThreshhold, ...): DSR_E_PARAMETER for an accumulator kind
 *                      other than 0 (MeanAcc) or 1 (VarianceAcc) and for lhoodThreshold != 0, DSR_E_DIMENSION for meanLen != 0 and
 *                      != featLen (extended means).  Host only
 *   speaker_list_read  SpeakerList (tr:1989-1998): one label a line, read with fgets into 128 bytes (a longer line arrives in pieces);
 *                      labels [*bytes] receives them joined by '\n' when cap suffices; DSR_E_PARSE for an empty line.  Host only
 *   create             S speaker slots over the trainer's model; massThreshold 0 means 10 (sat:1768); (nParts, part) pick the codebooks
 *                      as dsr_train_update does.  The trainer and its dsr_gmm must outlive the handle
 *   zero               SATMean::zero / SATVariance::zero of every Gaussian: the sums and occupancies; allocated blocks stay allocated
 *   set_stats          count - denCount, sumO and sumOsq of a trainer's accumulators into slot s (device to device);  set_stats_arrays
 *                      the same from host arrays c [G], sumO, sumOsq [G][dimN];  clear_slot  zero statistics and no transforms
 *   set_tree           the slot's transforms from an MLLR parameter tree, class by class (tr:2125-2135): DSR_E_DIMENSION for a matrix or
 *                      bias of another size (tr:1757-1761);  set_apt  from slot aptSlot of an APT handle through k_apt_matrix (the errors of
 *                      dsr_apt_get_matrix);  set_transform  from arrays: kind 1 (MLLR: the float chain of tr:1777-1784 in the variance
 *                      accumulator) or 2 (APT: the double sum stored to float, then the float bias, tr:1300-1336), A [nBlocks][bl][bl] with
 *                      bl = dimN / nBlocks, b [dimN] or NULL.  DSR_E_INDEX for class 0 (tr:2021-2022), DSR_E_DIMENSION for a block count that
 *                      does not divide dimN (sat:63-65) or bl > 81 (two bl^2 fp64 matrices in LDS).  set_tree and set_apt replace the
 *                      slot's transforms, set_transform adds or replaces one class
 *   set_apt_sub_features  nSubFeat of the RAPT / SLAPT files estimate_files reads (default 1)
 *   accumulate         what 1: SATMean::accumulate (sat:171-218), what 2: SATVariance::accumulate (sat:704-729), of slots 0 .. nSlots - 1 in
 *                      order for every Gaussian of the part, with the slot's transformer of exactly the Gaussian's class
 *                      (tr:2165-2173): DSR_E_INDEX for class 0, DSR_E_KEY for a missing class, DSR_E_CONSISTENCY for a class with a
 *                      descendant in the slot (not a leaf), DSR_E_DIMENSION for transforms of different block counts or another count than
 *                      an earlier batch's (sat:57-59; one count per handle, where the reference keeps one per Gaussian); nothing is
 *                      accumulated then.  float c = float(count - denCount); c == 0 contributes nothing and allocates no blocks.  The mean
 *                      sums are fp64 on v_mfma_f64_16x16x4_f64 in a fixed order (the same calls twice give the same bits), occ the
 *                      sequential double sum in slot order; the variance sums are the reference's arithmetic bit for bit
 *   update             what 1: MeanAcc::update (sat:1010-1023, 288-342): a Gaussian with occ < massThreshold is left alone; occ == 0 with
 *                      blocks zeroes the mean; otherwise per block auxOld, the solve (sat:257-274, component k kept when
 *                      |l_k| / max |l| >= 1e-7), auxNew, and the block kept as it was when auxOld < auxNew.  info [4] = ttlBlocks,
 *                      ttlBlocksUpdated, ttlDimensions, ttlDimensionsUpdated of this call (sat:304, 324, 339, 267, 273), totals [2] =
 *                      _TotalGaussians, _TotalUpdatedGaussians, *aux the sum of the per-block auxiliary values in model order.  A Gaussian
 *                      whose statistics are not finite or whose eigen-decomposition did not converge keeps its mean and is flagged
 *                      (gaussian_status); the others are done and the call returns DSR_E_CONSISTENCY; a NaN solution DSR_E_NUMERIC
 *                      what 2: VarianceAcc::update (sat:1233-1244, 731-756): below the threshold var = 1 / var (fixup), occ == 0 zeros,
 *                      otherwise float(vec / occ), a NaN DSR_E_NUMERIC.  The covariance slot holds VARIANCES afterwards: call
 *                      dsr_train_invert_variances and dsr_train_fix_gconsts.  Any of info, totals, aux may be NULL
 *   estimate_files     SATBase::estimate (sat:1802-1839): for every label of the list, in order, <accuPrefix><label>.cbs.accu is loaded
 *                      into the trainer (factor 1, the handle's nParts and part), <paramPrefix><label> (no separator, sat:1890) is read
 *                      as an MLLR tree or as RAPT / SLAPT parameters, S speakers are accumulated a batch, the trainer's accumulators are
 *                      zeroed; then update.  *ret = (sum totalPr) / (sum totalT).  The SAT accumulators are not zeroed first
 *   get_mean_accu      mat [bl][bl], vec [bl], scalar and occ of (Gaussian, block);  get_mean_accus  all [G][nBlocks][bl^2 + bl + 1], occ [G]
 *                      and the blocks-allocated flags [G];  get_var_accu(s)  vec [dimN] and occ.  Any pointer may be NULL
 *   keep_transformed   the next variance accumulations keep transform(origMean) of their slots;  get_transformed  [G][dimN] of slot s
 *   get_records        of the last mean update, [G][nBlocks]: kept dimensions, decision (0 left alone, 1 updated, 2 old mean kept,
 *                      3 zeroed, 4 flagged, 5 NaN), auxOld, auxNew;  get_solution  [G][dimN]: the solved means in double, before the
 *                      decision and the store to float (0 where nothing was solved);  gaussian_status  0, DSR_E_CONSISTENCY or DSR_E_NUMERIC
 *   kernel_ms          milliseconds of the last k_sat_mean_acc, k_sat_var_acc and k_sat_solve */
typedef struct dsr_sat dsr_sat;
dsr_status dsr_sat_check(int meanLen, int featLen, double lhoodThreshold, int accKind);
dsr_status dsr_speaker_list_read(const char* fileName, char* labels, int cap, int* n, int* bytes);
dsr_status dsr_sat_create(dsr_train*, int S, double massThreshold, int nParts, int part, dsr_sat** out);
void dsr_sat_destroy(dsr_sat*);
int dsr_sat_num_slots(const dsr_sat*);
int dsr_sat_num_blocks(const dsr_sat*);
dsr_status dsr_sat_set_apt_sub_features(dsr_sat*, int nSubFeat);
dsr_status dsr_sat_zero(dsr_sat*);
dsr_status dsr_sat_set_stats(dsr_sat*, int s, dsr_train*);
dsr_status dsr_sat_set_stats_arrays(dsr_sat*, int s, const double* c, const double* sumO, const double* sumOsq);
dsr_status dsr_sat_set_tree(dsr_sat*, int s, const dsr_param_tree*);
dsr_status dsr_sat_set_apt(dsr_sat*, int s, dsr_apt*, int aptSlot);
dsr_status dsr_sat_set_transform(dsr_sat*, int s, unsigned rc, int kind, int nBlocks, const double* A, const double* b);
dsr_status dsr_sat_get_transform(const dsr_sat*, int s, unsigned rc, int* kind, int* nBlocks, int* bSize, double* A, double* b);
int dsr_sat_slot_classes(const dsr_sat*, int s, unsigned* classes, int cap);
dsr_status dsr_sat_clear_slot(dsr_sat*, int s);
dsr_status dsr_sat_accumulate(dsr_sat*, int what, int nSlots, void* stream);
dsr_status dsr_sat_update(dsr_sat*, int what, unsigned info[4], unsigned totals[2], double* aux);
dsr_status dsr_sat_estimate_files(dsr_sat*, int what, const char* speakerList, const char* paramPrefix, const char* accuPrefix, double* ret);
dsr_status dsr_sat_get_mean_accu(dsr_sat*, int g, int block, double* mat, double* vec, double* scalar, double* occ);
dsr_status dsr_sat_get_mean_accus(dsr_sat*, double* acc, double* occ, int32_t* has);
dsr_status dsr_sat_get_var_accu(dsr_sat*, int g, double* vec, double* occ);
dsr_status dsr_sat_get_var_accus(dsr_sat*, double* vec, double* occ);
dsr_status dsr_sat_keep_transformed(dsr_sat*, int on);
dsr_status dsr_sat_get_transformed(dsr_sat*, int s, float* means);
dsr_status dsr_sat_get_records(const dsr_sat*, int32_t* kept, int32_t* decision, double* auxOld, double* auxNew);
dsr_status dsr_sat_get_solution(const dsr_sat*, double* means);
int dsr_sat_gaussian_status(const dsr_sat*, int g);
dsr_status dsr_sat_set_timing(dsr_sat*, int on);
dsr_status dsr_sat_kernel_ms(const dsr_sat*, float ms[3]);

/* ---------------------------------------------------------------------------------------------------------------------------------------
 * 14b. Fast speaker-adaptive training: fast accumulators, MDL means and the joint variance update (csrc/fsat_kernels.hip, csrc/fsat.cpp)
 *
 *    Replaces CodebookFastSAT::FastAccu, GaussDensity::normFastAccu / descLen and CodebookSetFastSAT (asr/sat/codebookFastSAT.cc, "cfs":
 *    135-254, 346-418, 523-539, 597-717), MDLSATMean (asr/sat/sat.cc, "sat": 383-493), FastSAT (sat:496-587), SATBase::FastAcc
 *    (sat:1028-1104) and SATFast<FastAcc> = FastMeanVarianceSAT (sat.h:803-844) for the model scope of section 14.  A dsr_fsat owns a
 *    dsr_sat: its S speaker slots and transform tables are those of section 14, and the SAT sums (mat, vec, scalar, occ, varVec) live in it.
 *    The training pass folds every speaker's sumO / sumOsq into one speaker-independent fast accumulator per Gaussian (norm), kept in one file
 *    that shards can sum (save_fast / load_fast); the estimation pass then needs only every speaker's counts and transforms (accumulate) and
 *    re-estimates means and variances together (update).
 *    Not implemented: fast accumulators of more than one class per Gaussian (subN > 1: replaceRegClass, ClassTotals, RegClassAcc /
 *    MMIRegClassAcc), MMIAcc / FastMMISAT, SATMeanFullCovar, cluster.cc, extended means (olen != featLen), an ldaFile.
 *
 *   check              the options of FastMeanVarianceSAT(cbs, meanLen, lhoodThreshhold, massThreshhold, nParts, part, mmiMultiplier,
 *                      meanOnly, maxNoRegClass) (sat.i:164-190): DSR_E_DIMENSION for extended means, DSR_E_PARAMETER for mmiMultiplier != 1
 *                      and maxNoRegClass != 1, which FastAcc ignores: refused rather than ignored.  Host only
 *   create             S speaker slots over the trainer's model; lhoodThreshold may be 0, massThreshold 0 means 10 (sat:1768), meanOnly is
 *                      SATBase::MeanOnly (sat:555-558).  The trainer and its dsr_gmm must outlive the handle.  sat: the dsr_sat inside,
 *                      borrowed: its transforms, sums, records, solution, statuses, timing and dsr_sat_set_apt_sub_features are read and set
 *                      through section 14; statistics go into a slot through the entries below only, which also keep numProb and denProb
 *   set_stats          count, denCount, sumO and sumOsq of a trainer's accumulators into slot s (device to device);  set_counts  the counts
 *                      alone (what a countsOnly accumulator file holds): enough for accumulate, refused by norm;  set_stats_arrays  from
 *                      host arrays count, denCount [G] and sumO, sumOsq [G][dimN], or both NULL for counts alone
 *   set_tree, set_apt, set_transform, clear_slot   as dsr_sat_* on the slot
 *   set_reg_classes_to_one   CodebookSetFastSAT::setRegClassesToOne (cfs:708-717): a Gaussian of class 0, or a model without classes,
 *                      gets class 1
 *   norm               CodebookSetFastSAT::normFastAccus (cfs:677-705) of slots 0 .. nSlots - 1 in order, for every Gaussian of the model:
 *                      set_reg_classes_to_one; the first call after creation or zero_fast allocates and zeroes the fast accumulators
 *                      (_zeroFastAccs); then GaussDensity::normFastAccu (cfs:346-418) with the slot's transformer of exactly the Gaussian's
 *                      class: count += numProb and denCount += denProb unless both are zero; unless |ck| < 1e-6 (ck = numProb - denProb, a
 *                      double), per block fastMean += (A o iv)^T (sumO - ck b), scalar += sum_m iv v^2 / ck, fastVar += sumOsq - 2 trn sumO
 *                      + ck trn^2 with trn = transform(origMean) in the transform's own types.  Sequential fp64 in the reference's order:
 *                      bit for bit.  One fast accumulator per Gaussian (subN == 1): DSR_E_KEY for a missing class, DSR_E_CONSISTENCY for a
 *                      class with a descendant in the slot (not a leaf) and for a slot that holds counts only, DSR_E_DIMENSION for
 *                      transforms of different block counts or another count than the accumulators'; nothing is added then.
 *                      DSR_E_NUMERIC ("Scalar is NaN.", cfs:407-408) after the fold
 *   zero_fast          the next norm, load_fast or set_fast allocates and zeroes;  fast_blocks  nblks of the fast accumulators, 0: none
 *   save_fast          CodebookSetFastSAT::saveFastAccus (cfs:597-617): the AccMap directory, then per codebook with a non-zero count the
 *                      Accu record of codebookTrain.cc:299-346 with countsOnly = 0 (name, refN, dimN, subN = 1, type, 0), orgDimN, nblks,
 *                      per Gaussian count, denCount, fastMean, fastVar, then the scalars [refN][nblks], the marker: big-endian floats
 *   load_fast          CodebookSetFastSAT::loadFastAccus (cfs:619-644) for the codebooks of (nParts, part): the file is ADDED.  A handle
 *                      without fast accumulators takes the file's nblks.  DSR_E_DIMENSION for another refN, dimN, subN, type, orgDimN or
 *                      nblks, DSR_E_CONSISTENCY for a counts-only record, DSR_E_IO for a truncated file or a missing marker; a refused
 *                      file leaves the accumulators as they were
 *   get_fast, set_fast count, denCount [G], fastMean, fastVar [G][dimN], scalar [G][nblks] in double; get: any pointer may be NULL
 *   add_fast           SATFast::addFastAccs (sat.h:833-842) for the Gaussians of the part: vec += fastMean, varVec += fastVar, scalar +=
 *                      fastScalar; every block counts as allocated afterwards
 *   accumulate         FastAcc::accumulate / FastSAT::accumulate (sat:1067-1077, 501-528) of slots 0 .. nSlots - 1: mat += c (A o iv)^T A
 *                      and occ += c with float c = float(count - denCount); sumO is never read.  The refusals of dsr_sat_accumulate.  It is
 *                      k_sat_mean_acc without its vec columns and its scalar pass: mat and occ have the bits dsr_sat_accumulate(1) gives
 *   update             FastAcc::update (sat:1079-1099): occ < massThreshold: var = 1 / var, the mean stays.  Otherwise the variances first
 *                      (float(varVec / occ), a NaN keeps 1 / var; 1 / var under meanOnly), then MDLSATMean::update (sat:395-493) per block:
 *                      auxOld = aux(mean) + thr descLen; M = V diag(l) V^T; t = V^T vec; component k kept when 0.5 t_k^2 / l_k > thr and
 *                      l_k / max(0, max l) >= 1e-7; x = V t'; auxNew = aux(x) + thr kept; auxOld < auxNew keeps the block and its descLen,
 *                      otherwise descLen = kept and the mean becomes float(x).  occ == 0 zeroes the mean.  info, totals, aux as
 *                      dsr_sat_update(1).  A Gaussian without blocks (nothing accumulated, no add_fast) is left as it is.  A Gaussian whose
 *                      statistics are not finite or whose eigen-decomposition did not converge keeps its mean and description lengths and
 *                      is flagged, its covariance slot becomes 1 / var like the rest; the others are done and the call returns
 *                      DSR_E_CONSISTENCY.  The covariance slot holds VARIANCES afterwards: call dsr_train_invert_variances and
 *                      dsr_train_fix_gconsts
 *   zero               dsr_sat_zero of the SAT sums (the fast accumulators and description lengths stay)
 *   desc_length        CodebookSetFastSAT::descLength (cfs:654-673): the sum over every (Gaussian, block); every block starts at 1
 *                      (cfs:523-539).  desc_blocks: the block count they are kept for, fixed by the first norm, load_fast, set_fast,
 *                      add_fast, accumulate or set_desc_len; 0 before (desc_length is then G x nSubFeat);  get_desc_len / set_desc_len
 *                      [G][nBlocks]
 *   estimate_files     SATFast::estimate (sat.h:825-831): add_fast, then SATBase::estimate (sat:1802-1839) as dsr_sat_estimate_files with
 *                      the matrix-only accumulate and this update; the speaker files may be counts-only or full (only the counts are
 *                      read).  *ret = (lhoodThreshold desc_length() + sum totalPr) / (sum totalT), desc_length taken before the update.  The
 *                      SAT sums are not zeroed first
 *   get_records        dsr_sat_get_records of the last update, and descLen [G][nBlocks] as that update left them
 *   kernel_ms          milliseconds of the last k_fsat_norm, matrix-only k_sat_mean_acc and k_fsat_solve (dsr_sat_set_timing on sat) */
typedef struct dsr_fsat dsr_fsat;
dsr_status dsr_fsat_check(int meanLen, int featLen, double massThreshold, double mmiMultiplier, int meanOnly, int maxNoRegClass);
dsr_status dsr_fsat_create(dsr_train*, int S, double lhoodThreshold, double massThreshold, int nParts, int part, int meanOnly, dsr_fsat** out);
void dsr_fsat_destroy(dsr_fsat*);
dsr_sat* dsr_fsat_sat(dsr_fsat*);
int dsr_fsat_fast_blocks(const dsr_fsat*);
int dsr_fsat_desc_blocks(const dsr_fsat*);
dsr_status dsr_fsat_set_stats(dsr_fsat*, int s, dsr_train*);
dsr_status dsr_fsat_set_counts(dsr_fsat*, int s, dsr_train*);
dsr_status dsr_fsat_set_stats_arrays(dsr_fsat*, int s, const double* count, const double* denCount, const double* sumO, const double* sumOsq);
dsr_status dsr_fsat_set_tree(dsr_fsat*, int s, const dsr_param_tree*);
dsr_status dsr_fsat_set_apt(dsr_fsat*, int s, dsr_apt*, int aptSlot);
dsr_status dsr_fsat_set_transform(dsr_fsat*, int s, unsigned rc, int kind, int nBlocks, const double* A, const double* b);
dsr_status dsr_fsat_clear_slot(dsr_fsat*, int s);
dsr_status dsr_fsat_set_reg_classes_to_one(dsr_fsat*);
dsr_status dsr_fsat_norm(dsr_fsat*, int nSlots, void* stream);
dsr_status dsr_fsat_zero_fast(dsr_fsat*);
dsr_status dsr_fsat_save_fast(dsr_fsat*, const char* fileName);
dsr_status dsr_fsat_load_fast(dsr_fsat*, const char* fileName, int nParts, int part);
dsr_status dsr_fsat_get_fast(dsr_fsat*, double* count, double* denCount, double* fastMean, double* fastVar, double* scalar);
dsr_status dsr_fsat_set_fast(dsr_fsat*, int nBlocks, const double* count, const double* denCount, const double* fastMean, const double* fastVar,
                             const double* scalar);
dsr_status dsr_fsat_add_fast(dsr_fsat*);
dsr_status dsr_fsat_accumulate(dsr_fsat*, int nSlots, void* stream);
dsr_status dsr_fsat_update(dsr_fsat*, unsigned info[4], unsigned totals[2], double* aux);
dsr_status dsr_fsat_zero(dsr_fsat*);
dsr_status dsr_fsat_desc_length(const dsr_fsat*, unsigned* dl);
dsr_status dsr_fsat_get_desc_len(const dsr_fsat*, uint16_t* descLen);
dsr_status dsr_fsat_set_desc_len(dsr_fsat*, int nBlocks, const uint16_t* descLen);
dsr_status dsr_fsat_estimate_files(dsr_fsat*, const char* speakerList, const char* paramPrefix, const char* accuPrefix, double* ret);
dsr_status dsr_fsat_get_records(const dsr_fsat*, int32_t* kept, int32_t* decision, double* auxOld, double* auxNew, int32_t* descLen);
dsr_status dsr_fsat_kernel_ms(const dsr_fsat*, float ms[3]);

#ifdef __cplusplus
}
#endif
#endif /* DSR_H */
