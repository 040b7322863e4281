/*
 * llsm_gpu.h -- batch / device-resident entry points of libllsm2_amd.
 *
 * ADDITIVE to the reference API (SURVEY.md section 8b "Extra the replacement
 * needs"): the reference analyses one utterance per llsm_analyze call
 * (layer0.c:478); a GPU wants thousands of utterances per launch and wants
 * them to stay in HBM between analysis and synthesis.  llsm_analyze /
 * llsm_synthesize (llsm.h) are thin wrappers over a batch of one.
 *
 * Plain C ABI: pointers and sizes only.  All functions returning int return 0
 * on success and a negative value on failure; llsm_gpu_last_error() holds the
 * message.  Nothing here falls back to the CPU.
 */
#ifndef LLSM_AMD_LLSM_GPU_H
#define LLSM_AMD_LLSM_GPU_H

#include <stddef.h>
#include "llsm.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct llsm_gpu_context llsm_gpu_context;
typedef struct llsm_gpu_batch   llsm_gpu_batch;

int         llsm_gpu_device_count(void);
const char* llsm_gpu_last_error(void);

/* `stream` is a hipStream_t handed over as void* (e.g. torch's current
 * stream) or NULL to let the context create its own. */
llsm_gpu_context* llsm_gpu_create_context(int device, void* stream);
void              llsm_gpu_delete_context(llsm_gpu_context* ctx);
void*             llsm_gpu_context_stream(llsm_gpu_context* ctx);
int               llsm_gpu_synchronize(llsm_gpu_context* ctx);

/* Conventions of the un-vendored ciglet primitives that the reference's own code cannot confirm (DESIGN.md
 * section 6).  Process-wide; read by contexts and batches at each call (below), by llsmrt buffers
 * when they are created.
 *   "hann_periodic"       0 (default): overlap-add Hann windows use the symmetric definition (n - 1); 1: periodic (n)
 *   "moving_avg_half"     3 (default): moving_avg(x, n, 3) averages 7 taps; 1: 3 taps
 *   "filtfilt_pad"        15 (default, 3 x the 5 coefficients): samples of odd extension at both ends (1 .. 15)
 *   "interp1u_exclusive"  0 (default): interp1u's samples span [x0, x1]; 1: [x0, x1)
 *   "kalman_init"         0 (default): kalmanf1d starts from x0 = z0, P0 = R0; 1: prior (z0, R0) followed by the filter
 *                         update of the first frame as well (P0 = (1 - K)(R0 + Q0))
 *   "spec2env_lobe_1e6"   cig_spec2env's constant (layer 1: log envelope raised so that the lobe peaks of a flat harmonic
 *                         spectrum sit on it) in units of 1e-6; 133979 (default) = the calibrated 0.13397922601295542
 *   "lf_rd_clamp"         lfmodel_from_rd: 0 (default) Fant's Rd regression with the usual extension formulas outside
 *                         0.21 <= Rd <= 2.7; 1: Rd limited to the range the regression was fitted on (0.3 .. 2.7) first
 * The CPU oracle has the same switches (oracle.h o_set_convention); set returns 0 or -1, get the value or -1.
 * A batch follows the conventions in force at each call: a batch created (or last used) under other values rebuilds
 * the tables it bakes them into -- windows, filter padding -- on its next llsm_gpu_batch_analyze / _synthesize, and
 * gives what a batch created under the new values gives, bit for bit. */
int llsm_gpu_set_convention(const char* name, int value);
int llsm_gpu_get_convention(const char* name);

/* Device memory of deleted batches is kept in a per-device cache (bounded by
 * $LLSM_GPU_POOL_MB, default 8192; 0 disables it) so that per-utterance hosts do
 * not pay ~30 hipMalloc/hipFree pairs on every llsm_analyze / llsm_synthesize
 * call.  This returns the cached blocks of the current device to the driver. */
void llsm_gpu_release_cached_memory(void);

/* Per-kernel HIP-event timing of every launch made through the context
 * (used by bench.py for the roofline object).  Off by default. */
int llsm_gpu_set_profiling(llsm_gpu_context* ctx, int enabled);
/* Events around the launches of ONE kernel name only (NULL / "": every kernel again); llsm_gpu_set_profiling(ctx, 2) switches the
 * events on and keeps this filter, (ctx, 1) clears it.  Events are recorded on the stream of the launch, so the analysis keeps its
 * second stream while profiling. */
int llsm_gpu_profile_only(llsm_gpu_context* ctx, const char* kernel_name);
int llsm_gpu_reset_profile(llsm_gpu_context* ctx);
/* Fills up to `cap` entries; returns the number of distinct kernels. */
int llsm_gpu_get_profile(llsm_gpu_context* ctx, int cap, const char** names,
  double* total_ms, int* launches);

/* Diagnostic for the register-resident wavefront FFT every spectral kernel is
 * built on (csrc/wave_fft.h): `count` independent complex transforms of
 * 2^logn points (logn in [8, 12]), interleaved re/im float host buffers,
 * forward (e^{-j}, unnormalised) or inverse (unscaled).  Returns 0 on success. */
int llsm_gpu_fft_selftest(llsm_gpu_context* ctx, int logn, int count, int inverse,
  const float* in, float* out);

/* Shape of a batch: utterance u owns samples [x_off[u], x_off[u]+nx[u]),
 * frames [frm_off[u], frm_off[u]+nfrm[u]) and output samples
 * [y_off[u], y_off[u]+ny[u]) of the flat arrays below. */
typedef struct {
  int n_utt;
  int total_samples;   /* sum nx   */
  int total_frames;    /* sum nfrm */
  int total_out;       /* sum ny, ny = round((nfrm+1)*thop*fs) (layer0.c:643) */
  int maxnhar, maxnhar_e, npsd, nchannel;
  int ntemplate_ext;   /* per (utterance, channel) white-noise template length */
} llsm_gpu_layout;

/* Flat arrays of a batch (row-major; F = total_frames). */
enum {
  LLSM_GPU_X = 0,        /* float [total_samples]        input waveform          */
  LLSM_GPU_F0,           /* float [F]                    (refined) F0            */
  LLSM_GPU_NHAR,         /* int   [F]                                            */
  LLSM_GPU_AMPL,         /* float [F][maxnhar]                                   */
  LLSM_GPU_PHSE,         /* float [F][maxnhar]                                   */
  LLSM_GPU_PSD,          /* float [F][npsd]              dB                      */
  LLSM_GPU_PSDRES,       /* float [F][npsd]              LLSM_FRAME_PSDRES       */
  LLSM_GPU_EDC,          /* float [F][nchannel]                                  */
  LLSM_GPU_NHAR_E,       /* int   [F]                                            */
  LLSM_GPU_EENV_AMPL,    /* float [F][nchannel][maxnhar_e]                       */
  LLSM_GPU_EENV_PHSE,    /* float [F][nchannel][maxnhar_e]                       */
  LLSM_GPU_XRES,         /* float [total_samples]        x - harmonic resynthesis*/
  LLSM_GPU_Y,            /* float [total_out]                                    */
  LLSM_GPU_YSIN,         /* float [total_out]                                    */
  LLSM_GPU_YNOISE,       /* float [total_out]                                    */
  LLSM_GPU_WHITE,        /* float [n_utt][nchannel][ntemplate_ext] Gaussian templates */
  LLSM_GPU_HAS_PSDRES,   /* int   [F]                    frame carries PSDRES    */
  /* layer-1 members, present after llsm_gpu_batch_enable_layer1 (nspec = nfft / 2 + 1) */
  LLSM_GPU_RD,           /* float [F]                    LLSM_FRAME_RD           */
  LLSM_GPU_VTMAGN,       /* float [F][nspec]             LLSM_FRAME_VTMAGN, dB   */
  LLSM_GPU_VSPHSE,       /* float [F][maxnhar]           LLSM_FRAME_VSPHSE       */
  LLSM_GPU_NVSPHSE,      /* int   [F]                    length of VSPHSE; 0: no layer-1 members */
  LLSM_GPU_PBPSYN,       /* int   [F]                    LLSM_FRAME_PBPSYN       */
  LLSM_GPU_HAS_HM,       /* int   [F]                    AMPL / PHSE / NHAR rows valid (LLSM_FRAME_HM present) */
  /* present after llsm_gpu_batch_enable_coder */
  LLSM_GPU_CODE,         /* float [F][order_spec + order_bap + 3]  frame-coder vectors   */
  LLSM_GPU_NARRAYS
};

/* options->thop, fs fix every window / FFT size of the batch.  nx, nfrm:
 * n_utt entries each. */
llsm_gpu_batch* llsm_gpu_create_batch(llsm_gpu_context* ctx,
  const llsm_aoptions* options, FP_TYPE fs, int n_utt, const int* nx,
  const int* nfrm);
void llsm_gpu_delete_batch(llsm_gpu_batch* b);
int  llsm_gpu_batch_layout(llsm_gpu_batch* b, llsm_gpu_layout* dst);
/* offsets: n_utt+1 entries each (may be NULL) */
int  llsm_gpu_batch_offsets(llsm_gpu_batch* b, int* x_off, int* frm_off, int* y_off);

/* Frequency axis of the PSD / PSDRES rows: they span linspace(0, fnyq, npsd) (LLSM_CONF_FNYQ,
 * layer0.c:578).  Defaults to fs / 2 (what llsm_analyze stores); a batch that synthesises parameters
 * analysed at another sampling rate sets the analysis Nyquist here (layer0.c:606-607 interpolates the
 * stored PSD onto the synthesis rate's bins). */
int  llsm_gpu_batch_set_fnyq(llsm_gpu_batch* b, FP_TYPE fnyq);

/* y = y_sin + y_noise on the HOST, bit for bit what the device holds in its y row (one float addition per sample,
 * layer0.c:657-659): a host that has downloaded the two parts forms the sum here instead of moving a third waveform
 * over the link (llsm_synthesize{,_batch} do so internally). */
void llsm_gpu_sum_outputs(FP_TYPE* y, const FP_TYPE* y_sin, const FP_TYPE* y_noise, long long n);

/* Diagnosis only: an intermediate plane of the batch, float32.
 * which = 0: the log envelope behind the Kalman process variance (layer0.c:339-343), 1: the log periodogram of the
 * residual (layer0.c:354-360); both [total_frames][nfft_psd / 2 + 1], of the last analysis.
 * which = 2: the squared band signals of the last analysis (llsm_subband_energy of x_res, or of x for a channel that
 * starts above 6 kHz; layer0.c:440), [nchannel][total_samples].
 * which = 3: the band-limited noise templates of the last synthesis (dsputils.c:385-394), [n_utt][nchannel][ntemplate_ext];
 * utterance u uses the first min(20000, ny[u]) + 128 samples of a row, and the rows of channels that start at or above
 * the synthesis Nyquist are never written (layer0.c:562 leaves such a channel out).
 * which = 4: the CMNDF plane of the last llsm_gpu_batch_estimate_f0 or llsm_gpu_batch_track_f0 of this batch that ran
 * with keep_cmndf = 1 (rule 5 below the former), [total_frames][lmax + 1] with that call's lmax; the row of a gated frame
 * is all ones.  Refused until such a call has run; no other call writes it.
 * which = 5: the candidate plane of the last llsm_gpu_batch_track_f0 of this batch (rule T1 below that call),
 * [total_frames][24]: f0[0..7], cost[0..7], l2[0..7] per frame.  Refused until such a call has run; no other call writes it.
 * which = 6: the distance planes of the last successful llsm_gpu_batch_align with this batch as a (rule D1 below that call):
 * pair after pair in list order, each [na][nb] row-major, sum of na x nb floats.  Refused until such a call has run; no
 * other call writes it.
 * which = 7 and 8: the candidate plane [total_frames][16] (rule S2 below llsm_gpu_batch_select) and the join plane
 * [total_frames][64] (rule S3) of the last successful llsm_gpu_batch_select with this batch as t.  Refused until such a
 * call has run; no other call writes them.
 * which = 9: the band planes of the last successful llsm_gpu_batch_align_band with this batch as a (rules B1 - B2 below that
 * call): pair after pair in list order, each [na][2 band + 1] row-major; entry q of row i is column c_i - band + q, and the
 * entries whose column lies outside [lo_i, hi_i] hold +infinity.  Refused until such a call has run; no other call writes
 * it, and that call does not write plane 6.
 * which = 10 and 11: the state plane [total_frames][32] and the join plane [total_frames][256] (below
 * llsm_gpu_batch_select_chain) of the last successful llsm_gpu_batch_select_chain with this batch as t.  Refused until
 * such a call has run, and again after an accepted call that failed; no other call writes them.
 * which = 12: the distance planes of the last successful llsm_gpu_batch_align_slope with this batch as a (rule L2 below that
 * call, which is D1): pair after pair in list order, each [na][nb] row-major, the whole matrix.  Refused until such a call
 * has run; no other call writes it, and that call writes neither plane 6 nor plane 9.
 * which = 13: the band planes of the last successful llsm_gpu_batch_align_band_slope with this batch as a (rules K1 - K2 below
 * that call), laid out as plane 9: pair after pair in list order, each [na][2 band + 1] row-major, entry q of row i column
 * c_i - band + q, +infinity where that column lies outside the band's row [p_i, q_i] (the whole band, not only the region of
 * K1).  Refused until such a call has run; no other call writes it, and that call writes none of planes 6, 9 and 12.
 * which = 14: the band planes of the last successful llsm_gpu_batch_align_around with this batch as a (rules A1 - A2 below that
 * call), laid out as plane 9 around that call's centre lines: pair after pair in list order, each [na][2 band + 1] row-major,
 * entry q of row i column c_i - band + q with c_i = center[pos0 + i], +infinity where that column lies outside [p_i, q_i].
 * Refused until such a call has run; no other call writes it, and that call writes none of planes 6, 9, 12 and 13.
 * which = 15: the noise excitation of the last llsm_gpu_batch_synthesize, [total_out] laid out as LLSM_GPU_YNOISE (utterance
 * after utterance at the batch's output offsets): the signal the noise filter of that call read.  Refused until a synthesis
 * has formed it; no other call writes it.
 * Each plane has its own length.  2 and 3 are refused (-1, with a message) until llsm_gpu_batch_analyze /
 * llsm_gpu_batch_synthesize has run the band filter on this batch.  The later stages of those calls only read the two
 * buffers and no other call writes them, so the planes stay valid until the next analyze / synthesize of the batch.
 * dst == NULL: only the size.  Returns the number of floats, -1 on error. */
long long llsm_gpu_batch_debug_plane(llsm_gpu_batch* b, int which, float* dst, long long cap);

/* Page-locked host buffers for the copies below (optional: any host pointer works, but
 * pageable memory is staged by the runtime and reaches a fraction of the PCIe rate). */
void* llsm_gpu_alloc_host(size_t bytes);
void  llsm_gpu_free_host(void* p);
/* Host-side placement.  llsm_gpu_device_numa_node: the NUMA node the device hangs off (sysfs `numa_node` of its PCI
 * function; -1 when the platform does not say).  llsm_gpu_bind_thread_to_device: binds the CALLING thread to that node's
 * CPUs (intersected with the CPUs it may already use) so that the staging copies into / out of page-locked blocks and the
 * blocks it allocates stay on the socket the PCIe link is on; returns the number of CPUs in the new mask, 0 if nothing was
 * changed (node unknown, no overlap, or $LLSM_GPU_NUMA_BIND=0).  The workers of the in-process fan-out call it on
 * themselves; a host that fills its own buffers may call it from the filling thread. */
int   llsm_gpu_device_numa_node(int device);
int   llsm_gpu_bind_thread_to_device(int device);

/* host <-> device copies of one flat array (whole array, host pointer) */
int   llsm_gpu_batch_upload(llsm_gpu_batch* b, int array_id, const void* src, size_t bytes);
int   llsm_gpu_batch_download(llsm_gpu_batch* b, int array_id, void* dst, size_t bytes);
/* The analysed rows FRAME-major: one record of llsm_gpu_batch_packed_words() 4-byte words per frame (layout: csrc/packed.h --
 * f0, nhar, nhar_e, has_psdres, then ampl | phse | psd | fparray header | psdres | edc | eenv_ampl | eenv_phse, every piece on
 * a 16-byte boundary), written by a kernel straight into PAGE-LOCKED host blocks, one per utterance: dst[u] receives the
 * nfrm[u] records of utterance u (dst itself page-locked: the kernel reads the table).  What llsm_analyze_batch uses to land
 * an utterance's frames in its chunk's slab without a staging copy; upload_packed is the other direction (asynchronous: the
 * synthesis launches follow on the stream); download_outputs writes y / y_sin / y_noise of utterance u to tab[3 u + 0 / 1 / 2]
 * (page-locked arrays of ny[u] samples; NULL entries skipped). */
int   llsm_gpu_batch_packed_words(llsm_gpu_batch* b);
int   llsm_gpu_batch_download_packed(llsm_gpu_batch* b, int n_utt, void* const* dst);
int   llsm_gpu_batch_upload_packed(llsm_gpu_batch* b, int n_utt, const void* const* src);
int   llsm_gpu_batch_download_outputs(llsm_gpu_batch* b, int n_utt, float* const* tab);
/* the records of the whole batch as ONE block through the copy engine (host: page-locked, total_frames x words x 4 bytes,
 * utterance u at frm_off[u] x words); upload is asynchronous */
int   llsm_gpu_batch_download_packed_block(llsm_gpu_batch* b, void* host);
int   llsm_gpu_batch_upload_packed_block(llsm_gpu_batch* b, const void* host);
/* several arrays in one call: all copies enqueued, the stream waited for once (to_device != 0: upload; same checks as the
 * single-array calls; the host buffers must stay valid until the call returns) */
int   llsm_gpu_batch_transfer_many(llsm_gpu_batch* b, int to_device, int n, const int* array_ids, void* const* host, const size_t* bytes);
/* The eleven parameter rows of a batch (LLSM_GPU_F0, NHAR, AMPL, PHSE, PSD, PSDRES, HAS_PSDRES, EDC, NHAR_E, EENV_AMPL,
 * EENV_PHSE) are pieces of ONE device block: params_layout reports its size, the byte offset of each piece and the array
 * id behind it (any output may be NULL); transfer_params moves the whole block in one copy to / from a host buffer laid out
 * with the same offsets (to_device != 0: upload).  One copy instead of eleven: a small device-to-host copy costs ~0.1 ms
 * whatever its size. */
int   llsm_gpu_batch_params_layout(llsm_gpu_batch* b, size_t* total_bytes, size_t* offsets11, int* array_ids11);
int   llsm_gpu_batch_transfer_params(llsm_gpu_batch* b, int to_device, void* host_block);
/* device address of a flat array (stays valid until the batch is deleted) */
void* llsm_gpu_batch_device_ptr(llsm_gpu_batch* b, int array_id);
size_t llsm_gpu_batch_array_bytes(llsm_gpu_batch* b, int array_id);

/* Enqueue layer-0 analysis of every utterance of the batch (inputs: X, F0;
 * outputs: F0 (refined), NHAR .. EENV_PHSE, XRES).  Asynchronous. */
int llsm_gpu_batch_analyze(llsm_gpu_batch* b);
/* Enqueue layer-0 synthesis from the parameter arrays currently resident in
 * the batch (outputs: Y, YSIN, YNOISE).  seed drives the counter-based
 * Gaussian generator; use_injected_white != 0 makes it read LLSM_GPU_WHITE
 * instead.  Asynchronous. */
int llsm_gpu_batch_synthesize(llsm_gpu_batch* b, const llsm_soptions* options,
  unsigned long long seed, int use_injected_white);

/* ---- layer 1 (source-filter model) on a device-resident batch; replaces layer1.c:129-195 ----
 * enable_layer1   allocates the layer-1 arrays (nfft: size of the vocal-tract response, power of two)
 * tolayer1        llsm_chunk_tolayer1 over every utterance: RD on every frame, VTMAGN / VSPHSE on voiced
 *                 frames (inputs: F0, NHAR, AMPL, PHSE; lip radius from the batch options)
 * tolayer0        llsm_frame_tolayer0 over every frame with layer-1 members (only_missing != 0: only frames
 *                 whose HAS_HM flag is 0); writes NHAR / AMPL / PHSE and sets HAS_HM
 * set_maxnhar_conf  LLSM_CONF_MAXNHAR as llsm_frame_tolayer0 reads it (layer1.c:166-167); < 0: absent
 * set_pbpeffect   LLSM_FRAME_PBPEFF of one frame: `modifier` is called on the host, in frame / pulse order,
 *                 while llsm_gpu_batch_synthesize (use_l1 = 1) schedules the pulses (layer0.c:208-217)
 * llsm_gpu_batch_synthesize with options->use_l1 = 1 then renders layer0.c:148-287 on the device. */
int llsm_gpu_batch_enable_layer1(llsm_gpu_batch* b, int nfft);
int llsm_gpu_batch_tolayer1(llsm_gpu_batch* b, int nfft);
int llsm_gpu_batch_tolayer0(llsm_gpu_batch* b, int only_missing);
int llsm_gpu_batch_set_maxnhar_conf(llsm_gpu_batch* b, int maxnhar_conf);
int llsm_gpu_batch_set_pbpeffect(llsm_gpu_batch* b, int frame, llsm_fgfm modifier, void* info,
  llsm_container* src_frame);

/* ---- edits of a device-resident batch: the middle of the reference's time-stretch recipe (analyse, tolayer1,
 * phasepropagate(-1), blend frames onto a new grid, tolayer0, phasepropagate(+1), synthesise) without leaving the device.
 * All three are asynchronous; a refused call returns -1, sets llsm_gpu_last_error() and launches nothing.
 *
 * phasesync_rps   llsm_chunk_phasesync_rps over every frame.  The reference phase of a frame is VSPHSE[0] if layer1_based
 *                 and NVSPHSE > 0, else PHSE[0] if the frame's HM rows are valid and NHAR > 0, else 0; the frame is shifted
 *                 by minus it.
 * phasepropagate  llsm_chunk_phasepropagate per utterance: frame i is shifted by
 *                 (float)((double)acc_i * ((double)(float)(thop * sign) * 2 pi)), acc_i the float32 inclusive running sum of
 *                 the utterance's F0 row in frame order.
 *   A shift by theta maps phase k (0-based) to wrap(phi + theta (k + 1)) in float64 (llsm_frame_phaseshift) on: the first
 *   NHAR entries of PHSE of voiced frames (F0 != 0) whose HM rows are valid (HAS_HM, when the batch has layer 1); the
 *   first NHAR_E entries of every channel of EENV_PHSE of voiced frames; the first NVSPHSE entries of VSPHSE.  Nothing
 *   else is written.  Both calls give rows bit-identical to the host functions on the same frames.
 *
 * retime          resamples every utterance of `src` (which it does not change) onto the frame grid of `dst`.  dst was
 *                 created with src's options and sampling rate and the same number of utterances, with frame counts of
 *                 its own (nx may be 0); src has layer 1 (llsm_gpu_batch_tolayer1).  dst gets layer 1 with src's nfft and
 *                 takes over src's fnyq and maxnhar_conf.
 *   pos         host, dst.total_frames floats: entry frm_off_dst[u] + i is the position of output frame i of utterance u in
 *               source frames of that utterance, within [0, nfrm_src[u] - 1].  NULL: the uniform map
 *               llsm_gpu_retime_uniform_positions(nfrm_src[u], nfrm_dst[u]).
 *   psdres_src  host, dst.total_frames source frame indices (of the utterance): output frame i takes PSDRES and HAS_PSDRES
 *               from that frame.  NULL: floor(pos).
 *   Output frame at position t of an utterance of n source frames: a = min(floor(t), n - 2), b = a + 1, r = t - a (float32).
 *   r == 0 or r == 1 (n == 1 included): a bit-exact copy of frame a or b.  Otherwise, with lin = x_a + (x_b - x_a) r in float32
 *   and circ = atan2(lin(sin), lin(cos)):
 *     both voiced  F0, RD lin; VTMAGN lin; VSPHSE circ over the first min(NVSPHSE) entries, the rest from the frame with the
 *                  longer row; NVSPHSE = max
 *     one voiced   F0, RD, VSPHSE, NVSPHSE of the voiced frame; VTMAGN its row + 20 log10(max(1e-8, w)) dB, w = r if b is the
 *                  voiced frame, 1 - r if a is
 *     neither      F0 = 0, RD = 1, layer-1 rows of frame a
 *     VTMAGN is floored at -80 dB; PSD, EDC lin; EENV_AMPL lin and EENV_PHSE circ over the first min(NHAR_E) entries of each
 *     channel, the rest from the longer frame, NHAR_E = max; PBPSYN of frame a; voiced output frames get NHAR = 0 and
 *     HAS_HM = 0 (llsm_gpu_batch_tolayer0(dst, 1) rebuilds them), unvoiced ones frame a's NHAR, AMPL, PHSE and HAS_HM.
 *   Per-frame effects (llsm_gpu_batch_set_pbpeffect) are not carried over.  An utterance's output depends on nothing else in
 *   the batch.  Refused: differing options or utterance counts, different contexts, src == dst, src without layer 1, a NaN
 *   or out-of-range position or psdres_src index, an utterance with frames on one side only, dst with layer 1 of another size.
 * retime_uniform_positions  host only: pos[i] = min((float)i * nfrm_src / nfrm_dst, nfrm_src - 1) in float32, i < nfrm_dst. */
int  llsm_gpu_batch_phasesync_rps(llsm_gpu_batch* b, int layer1_based);
int  llsm_gpu_batch_phasepropagate(llsm_gpu_batch* b, int sign);
int  llsm_gpu_batch_retime(llsm_gpu_batch* dst, const llsm_gpu_batch* src, const FP_TYPE* pos, const int* psdres_src);
void llsm_gpu_retime_uniform_positions(int nfrm_src, int nfrm_dst, FP_TYPE* pos);

/* ---- splice: a gather of frames across the utterances of another batch with a two-sided blend -- retiming, unit selection,
 * concatenation with cross-fades and morphing between two voices from index lists, without leaving the device.
 * Asynchronous on the context's stream; a refused call returns -1, sets llsm_gpu_last_error() (the message starts with
 * "llsm_gpu_batch_splice:" and names the frame at fault) and writes and launches nothing.
 *
 * src and dst share options, sampling rate, channel frequencies and context, as for retime; their utterance counts may
 * differ.  src has layer 1 and is only read.  dst gets layer 1 with src's nfft, takes over src's fnyq and maxnhar_conf,
 * and its lowest-F0 bound becomes unknown.  All arrays of the map are host arrays of dst.total_frames entries in dst's
 * flat frame order.
 *
 * With S[u][i] frame i of utterance u of src and P(fa, fb, r) the pair rule of retime above (r == 0: a bit-exact copy of
 * fa, r == 1: of fb, otherwise the both-voiced / one-voiced / neither rules with fa in the place of frame a), output
 * frame g is
 *     A = P(S[ua][a], S[ua][a + 1], ra)   ua = utt_a[g], and a = min(floor(t), n - 2), ra = t - a (float32) from
 *                                         t = pos_a[g] and the n frames of utterance ua, as retime forms them (n == 1: S[ua][0])
 *     B = the same from utt_b[g], pos_b[g]
 *     out = P(A, B, mix[g])
 *   so mix[g] == 0, or a map without a second side, gives A bit for bit -- AMPL, PHSE, NHAR and HAS_HM of an exactly copied
 *   frame included -- and mix[g] == 1 gives B bit for bit; a side the output does not use is not read.  In between, A and B
 *   enter P as the frames retime would have written for them (voiced blends with NHAR = 0, HAS_HM = 0 and zero AMPL /
 *   PHSE rows, NVSPHSE and NHAR_E clamped to the row widths).
 *   PSDRES and HAS_PSDRES are those of source frame min(floor(pos_a[g]), n - 1) of utt_a[g] when there is no second side
 *   or mix[g] < 0.5, else of the corresponding frame of utt_b[g].
 *   Per-frame effects are not carried over.  An output frame depends on its own map entries and the at most four source
 *   frames they name, not on its place in dst nor on anything else in either batch.
 * Refused: a NULL batch or map; pos_a NULL; a second side given in part; src == dst; different contexts, options or
 * sampling rates; src without layer 1; dst with layer 1 of another size; utt_a NULL while dst has more utterances than
 * src; an utterance index outside src; a named utterance without frames; a position that is NaN or outside
 * [0, nfrm - 1] of its utterance; a mix that is NaN or outside [0, 1].  A dst without frames returns 0. */
typedef struct {
  const int*     utt_a;  /* dst.total_frames source-utterance indices; NULL: the output frame's own utterance index */
  const FP_TYPE* pos_a;  /* dst.total_frames positions, in frames of utterance utt_a; required */
  const int*     utt_b;  /* the second side; utt_b, pos_b and mix are all NULL or all given */
  const FP_TYPE* pos_b;
  const FP_TYPE* mix;    /* weight of side b, in [0, 1] */
} llsm_gpu_splice_map;
int llsm_gpu_batch_splice(llsm_gpu_batch* dst, const llsm_gpu_batch* src, const llsm_gpu_splice_map* map);

/* ---- pitch and formant edit of a device-resident layer-1 batch: the middle of the reference's pitch-shift recipe
 * (analyse, tolayer1, phasepropagate(-1), F0 *= ratio and VTMAGN -= 20 log10(ratio) with HM dropped, tolayer0,
 * phasepropagate(+1), synthesise), with an optional formant warp of VTMAGN and PSD.  Asynchronous; a refused call returns
 * -1, sets llsm_gpu_last_error() and writes and launches nothing.
 *
 * f0_ratio, formant_ratio  host, total_frames floats each, in the batch's frame order; NULL: 1 on every frame.
 * flags                    0 or LLSM_GPU_WARP_PSD (the PSD row is warped too).
 * For frame g with rho = f0_ratio[g], alpha = formant_ratio[g]:
 *   rho == 1 and alpha == 1  the frame is not touched (every row bit for bit, HM included).
 *   unvoiced (F0 == 0)       F0 and the layer-1 rows are not touched; with LLSM_GPU_WARP_PSD and alpha != 1 the PSD row
 *                            is warped by alpha.  Nothing else changes.
 *   voiced, otherwise        F0' = F0 * rho in float32;
 *                            W = VTMAGN warped by alpha (an exact copy when alpha == 1);
 *                            VTMAGN'[k] = (float)((double)W[k] - 20 log10((double)rho)), the logarithm in float64, no floor;
 *                            NHAR = 0 and HAS_HM = 0, so that llsm_gpu_batch_tolayer0(b, 1) rebuilds the harmonics (the
 *                            AMPL and PHSE rows are not written); with LLSM_GPU_WARP_PSD and alpha != 1 the PSD row is
 *                            warped by alpha.  RD, VSPHSE, NVSPHSE, PBPSYN, PSDRES, EDC and EENV are not touched.
 *   Warp of a row x of n bins on linspace(0, fnyq, n) (VTMAGN: n = nspec, PSD: n = npsd), moving the envelope at f to
 *   alpha f: for each bin k, p = (double)k / (double)alpha (correctly rounded), i = floor(p); i >= n - 1: out[k] = x[n - 1];
 *   else out[k] = x[i] + (x[i + 1] - x[i]) r in float32 without contraction, r = (float)(p - i).
 * Refused: a NULL batch, a batch without layer 1, an unknown flag bit, a ratio that is NaN, infinite or outside its range
 * (rho in [1/16, 16], alpha in [1/4, 4]; the message names the frame), rows too long for the kernel's LDS
 * (nspec + npsd > 10240).  The batch's lowest-F0 bound follows the edit.
 * Known limit: tolayer0 caps the harmonics of a frame at NVSPHSE, as the reference does, so a downward shift by rho also
 * narrows the harmonic band by rho; VSPHSE is not extended. */
enum { LLSM_GPU_WARP_PSD = 1 };
int llsm_gpu_batch_pitch_formant(llsm_gpu_batch* b, const FP_TYPE* f0_ratio, const FP_TYPE* formant_ratio, int flags);

/* ---- smoothing of parameter tracks around joins: a triangular weighted mean along the frames of a layer-1 batch, in place,
 * of F0, RD, VTMAGN, PSD and EDC -- the tracks that step where llsm_gpu_batch_splice renders an index list of
 * llsm_gpu_batch_select that hops between recordings.  No phase row is touched and nothing is averaged in a logarithmic
 * domain.  Asynchronous on the context's stream; a refused call returns -1, sets llsm_gpu_last_error() (the message starts
 * with "llsm_gpu_batch_smooth:" and names the frame at fault) and writes and launches nothing.
 *
 * radius  host, total_frames ints in the batch's flat frame order: the reach of the mean of every frame, 0: not touched.
 * flags   an OR of LLSM_GPU_SMOOTH_*: the tracks that are smoothed.
 *
 * The rules, for frame g = frm_off[u] + i of an utterance u of n frames, with R = radius[g].  Every value read below is
 * the value the rows held BEFORE the call: the call works on a snapshot, never on a value it has just written.
 *  S1. R == 0: the frame is not touched, every row bit for bit, AMPL, PHSE, NHAR and HAS_HM included.
 *  S2. Frame j is voiced when F0[j] != 0.  The window starts as [max(0, i - R), min(n - 1, i + R)], frames of utterance u
 *      only: it never crosses into a neighbouring utterance of the flat arrays.  It is then shrunk from both ends to the
 *      largest interval around i in which every frame has frame i's voicing: a track is never averaged across a voicing
 *      change.  The result is [lo, hi], lo <= i <= hi.
 *  S3. lo == hi: the frame is not touched, as in S1.
 *  S4. The weights are w_j = R + 1 - |j - i| (integers >= 1) and W is their sum over j = lo ... hi.  For a track x,
 *          S(x) = (float)( (sum over j = lo ... hi of (double)w_j * (double)x_j) / (double)W ):
 *      the sum is float64, starts from 0.0 and runs over j ascending with one addition per term; every product is exact in
 *      float64, so contraction cannot change a bit; the division and the conversion to float32 are correctly rounded.  The
 *      order of the additions is part of the contract.
 *  S5. Voiced frame: F0, RD and every bin of VTMAGN become S(.) of their tracks where LLSM_GPU_SMOOTH_F0, _RD and _VTMAGN
 *      are set; there is no floor on VTMAGN.  If any of these three flags is set, NHAR = 0 and HAS_HM = 0, so that
 *      llsm_gpu_batch_tolayer0(b, 1) rebuilds the harmonics; the AMPL and PHSE rows are not written.  Every point of PSD
 *      and every channel of EDC become S(.) where LLSM_GPU_SMOOTH_PSD and _EDC are set.
 *  S6. Unvoiced frame: PSD and EDC as in S5 where flagged; nothing else changes.
 *  S7. Never written: VSPHSE, NVSPHSE, PSDRES, HAS_PSDRES, EENV_AMPL, EENV_PHSE, NHAR_E, PBPSYN, per-frame effects and the
 *      waveforms.
 *  S8. An output frame depends on its own radius and on the at most 65 frames of its own utterance in its window, and on
 *      nothing else in the batch: not on its place in the batch, on other radii or on earlier calls.
 *  S9. The batch's lowest-F0 bound stays as it is: a weighted mean of voiced F0 values, rounded monotonically, is never
 *      below their minimum.
 * Refused, every check before anything changes: a NULL batch or a NULL radius; a batch without layer 1; flag bits outside
 * LLSM_GPU_SMOOTH_ALL; a radius below 0 or above LLSM_GPU_SMOOTH_MAX_RADIUS; scratch that cannot be allocated.
 * Returns 0 without a launch: flags == 0, a batch without frames, a radius that is all zeros.
 *
 * llsm_gpu_join_radii  host only: the radius array from the utt_a / pos_a lists of a splice map (llsm_gpu_splice_map,
 *   llsm_gpu_batch_select).  nfrm holds the n_utt frame counts of the destination, utt_a and pos_a one entry per
 *   destination frame in flat order; utt_a NULL: every frame's source is its own utterance, as in the splice map.  In a
 *   destination utterance at flat offset o a join lies between frames i - 1 and i (1 <= i < n) unless
 *   utt_a[o + i] == utt_a[o + i - 1] and pos_a[o + i] == pos_a[o + i - 1] + 1 in float32 (the natural continuation of rule
 *   S3 of llsm_gpu_batch_select).  The distance of frame i to a join at i_j is i - i_j for i >= i_j and i_j - 1 - i below
 *   it, and radius[o + i] = max(0, reach - d) with d the least distance to a join of the utterance: the two frames at a
 *   join get reach and the radius falls by one per frame to 0; an utterance without joins gets zeros.  Returns the number
 *   of joins, or -1 with a message ("llsm_gpu_join_radii: ...") for a NULL nfrm, pos_a or radius, a negative count, or a
 *   reach outside [0, LLSM_GPU_SMOOTH_MAX_RADIUS]; radius is then untouched.
 * Known limit: the mean is linear in the rows' own units (VTMAGN in dB, F0 in Hz), and the window is cut, not faded, at a
 * voicing change. */
enum { LLSM_GPU_SMOOTH_F0 = 1, LLSM_GPU_SMOOTH_RD = 2, LLSM_GPU_SMOOTH_VTMAGN = 4,
       LLSM_GPU_SMOOTH_PSD = 8, LLSM_GPU_SMOOTH_EDC = 16, LLSM_GPU_SMOOTH_ALL = 31 };
enum { LLSM_GPU_SMOOTH_MAX_RADIUS = 32 };
int llsm_gpu_batch_smooth(llsm_gpu_batch* b, const int* radius, int flags);
int llsm_gpu_join_radii(int n_utt, const int* nfrm, const int* utt_a, const FP_TYPE* pos_a,
                        int reach, int* radius);   /* host only */

/* ---- F0 estimation: LLSM_GPU_X -> LLSM_GPU_F0 on the device, a YIN-style estimator (difference function, cumulative mean
 * normalised difference "CMNDF", first dip below a threshold, parabolic fit, median of five).  It is the estimator of
 * tests/golden/make_f0_track.py on the batch's frame grid and decides every frame alone; llsm_gpu_batch_track_f0 below
 * searches a path through the candidate dips of the same CMNDF rows.
 * Asynchronous on the context's stream; a refused call returns -1, sets llsm_gpu_last_error() (the message starts with
 * "llsm_gpu_batch_estimate_f0:") and writes and launches nothing.  The call reads LLSM_GPU_X and writes all total_frames
 * entries of LLSM_GPU_F0 and nothing else; afterwards the batch's lowest-F0 bound is unknown, as after every call that
 * writes the F0 row on the device (a full host upload of F0 makes it known again).
 *
 * The rules, per utterance with samples x[0, nx), nfrm frames and the batch's thop and fs; options enter as the float64
 * values of their float32 members, arithmetic is float64 unless stated:
 *  1. lmin = (int)(fs / fmax), lmax = (int)(fs / fmin); W = lmax + window_extra; nfft = the smallest power of two that is
 *     >= 256 and >= W + lmax.
 *  2. Frame i: c = round(i * thop * fs) as the analysis forms it (float32 products); s[n] = x[c - W / 2 + n] for n in
 *     [0, W + lmax), integer division, zero outside [0, nx).
 *  3. The frame is unvoiced (raw value 0) if sum_{n<W} s[n]^2 is 0 or sum_{n<W} s[n]^2 / W < silence_rel^2 * sum x^2 / nx; the
 *     utterance's sum of squares is taken in an order fixed by nx alone.
 *  4. d[tau] = sum_{n<W} (s[n] - s[n + tau])^2 for tau in [0, lmax] -- evaluated as E(0) + E(tau) - 2 r(tau) with
 *     E(tau) = sum_{n<W} s[n + tau]^2 and r the cross-correlation of s[0, W) with s; r comes from float32 transforms.
 *  5. cm[0] = 1, cm[tau] = d[tau] * tau / max(sum_{j=1..tau} d[j], 1e-12), kept as float32.
 *  6. The first tau in [lmin, lmax) with cm[tau] < threshold (none: raw value 0); then while tau + 1 < lmax and
 *     cm[tau + 1] < cm[tau]: tau ++.
 *  7. y0, y1, y2 = cm[tau - 1], cm[tau], cm[tau + 1]; den = y0 - 2 y1 + y2; off = 0.5 (y0 - y2) / den if |den| > 1e-12, else
 *     0; raw = (float)(fs / (tau + off)).
 *  8. smooth = 1, over the raw values of the utterance: for 2 <= i < nfrm - 2 with nz non-zero entries among
 *     raw[i - 2 .. i + 2]: raw[i] != 0 and nz >= 4: the median of the non-zero entries (of four: the float32 mean of the
 *     middle two); raw[i] != 0 and nz <= 2: 0; otherwise raw[i].  The first and last two frames keep their raw values.
 *     smooth = 0: the raw values.
 * A frame's value depends on its own utterance only: not on the batch, the utterance's place in it, or any other call.
 *
 * Refused: a NULL batch; a NaN option; fmin <= 0; fmin >= fmax; lmin < 2; lmax <= lmin + 1; threshold outside (0, 1];
 * silence_rel < 0; window_extra < 1; smooth or keep_cmndf not 0 or 1; W + lmax > 4096 (the largest transform); a batch
 * with frames but no samples.  A batch without frames returns 0.
 * llsm_gpu_f0_plan is host only: the sizes of rule 1 at fs (NULL pointers are skipped; opt NULL: the defaults); 0, or -1
 * with the message llsm_gpu_batch_estimate_f0 would give when it would refuse the options. */
typedef struct {
  FP_TYPE fmin, fmax;      /* search range in Hz; defaults 50, 500 */
  FP_TYPE threshold;       /* CMNDF threshold; default 0.15 */
  FP_TYPE silence_rel;     /* gate: window RMS below silence_rel x utterance RMS -> unvoiced; default 0.05 */
  int     window_extra;    /* integration window W = lmax + window_extra samples; default 200 */
  int     smooth;          /* 1 (default): the median-of-5 pass of rule 8; 0: raw values */
  int     keep_cmndf;      /* 1: keep the CMNDF plane for llsm_gpu_batch_debug_plane(b, 4, ...); default 0 */
} llsm_gpu_f0_options;
void llsm_gpu_f0_default_options(llsm_gpu_f0_options* dst);
int  llsm_gpu_f0_plan(const llsm_gpu_f0_options* opt, FP_TYPE fs, int* lmin, int* lmax, int* W, int* nfft);
int  llsm_gpu_batch_estimate_f0(llsm_gpu_batch* b, const llsm_gpu_f0_options* opt /* NULL: defaults */);

/* ---- F0 tracking: LLSM_GPU_X -> LLSM_GPU_F0 on the device, a minimum-cost path (Viterbi) per utterance through the
 * candidate dips of the CMNDF rows of llsm_gpu_batch_estimate_f0.  The estimator above takes the first dip below its
 * threshold, which is the octave above wherever the odd harmonics fade (a formant on 2 F0) for longer than its median
 * reaches; here every dip below cand_threshold is a candidate and continuity decides between them.  pYIN's probabilistic
 * thresholds and HMM are not provided.
 * Asynchronous on the context's stream; a refused call returns -1, sets llsm_gpu_last_error() (the message starts with
 * "llsm_gpu_batch_track_f0:") and writes and launches nothing.  The call reads LLSM_GPU_X and writes all total_frames
 * entries of LLSM_GPU_F0, scratch of its own (the candidate plane, llsm_gpu_batch_debug_plane(b, 5, ...), always kept) and
 * nothing else; afterwards the batch's lowest-F0 bound is unknown.
 * opt supplies fmin, fmax, silence_rel, window_extra and keep_cmndf to rules 1 - 5 above; its threshold and smooth are
 * checked as llsm_gpu_batch_estimate_f0 checks them and otherwise not read.  NULL: the defaults, for either struct.
 *
 * The rules, per utterance.  Rules 1 - 5 above give the float32 row cm[0 .. lmax] and the gate (rule 3) of each frame.
 *  T1. Candidates of a frame that is not gated: every lag tau in [lmin, lmax) with cm[tau] < cm[tau - 1], cm[tau] <=
 *      cm[tau + 1] and cm[tau] < cand_threshold (float32 comparisons).  The K = 7 of lowest cm[tau] are kept, ties to the
 *      smaller tau, and stored in that order: cost = cm[tau]; f0 = (float)(fs / (tau + off)) with off of rule 7 in float64;
 *      l2 = (float)log2((double)f0).  n <= 7 is their number; a gated frame has none.  L = (float)log2((double)fs / lmin).
 *      Row g of the candidate plane: f0[0..7], cost[0..7], l2[0..7]; slots n .. 6 are zero, f0[7] = cost[7] = 0, l2[7] = L.
 *  T2. Eight states per frame: the candidate slots 0 .. 6, and unvoiced (7).  From here on float32, one rounding per
 *      operation, no contraction.  loc[k] = cost[k] + octave_cost * (L - l2[k]) for k < n, +inf for n <= k < 7;
 *      loc[7] = unvoiced_cost if n > 0, else 0.
 *  T3. Transition from state a of frame i - 1 to state j of frame i: both voiced jump_cost * |l2_i[j] - l2_{i-1}[a]|; both
 *      unvoiced 0; otherwise switch_cost.
 *  T4. acc_0 = loc_0.  For i >= 1: acc_i[j] = min_a(acc_{i-1}[a] + tr(a, j)) + loc_i[j] over the a with finite acc_{i-1}[a],
 *      the back pointer of j the smallest a that attains the minimum; then the smallest acc_i[j] of the frame is
 *      subtracted from every acc_i[j].  The path ends in the smallest state of least acc on the last frame and follows the
 *      back pointers from there.
 *  T5. The F0 of frame i is f0_i[state], 0 for the unvoiced state.  There is no median pass.
 * A frame's value depends on its own utterance only: not on the batch, the utterance's place in it, or any other call.
 *
 * Refused: everything llsm_gpu_batch_estimate_f0 refuses; a NaN or infinite track option; cand_threshold outside (0, 1]; a
 * negative cost.  A batch without frames returns 0.
 * llsm_gpu_f0_track_check is host only: 0, or -1 with the message llsm_gpu_batch_track_f0 would give for these track
 * options (NULL: the defaults). */
typedef struct {
  FP_TYPE cand_threshold;  /* a local minimum of the CMNDF is a candidate if below this; default 0.5; (0, 1] */
  FP_TYPE unvoiced_cost;   /* local cost of the unvoiced state on a frame that has candidates; default 0.2; >= 0 */
  FP_TYPE switch_cost;     /* voiced <-> unvoiced transition; default 0.05; >= 0 */
  FP_TYPE jump_cost;       /* per octave between consecutive voiced frames; default 0.5; >= 0 */
  FP_TYPE octave_cost;     /* per octave below fs / lmin, added to a candidate's local cost; default 0.02; >= 0 */
} llsm_gpu_f0_track_options;
void llsm_gpu_f0_track_default_options(llsm_gpu_f0_track_options* dst);
int  llsm_gpu_f0_track_check(const llsm_gpu_f0_track_options* topt);
int  llsm_gpu_batch_track_f0(llsm_gpu_batch* b, const llsm_gpu_f0_options* opt, const llsm_gpu_f0_track_options* topt);

/* ---- alignment: one minimum-cost monotonic path (dynamic time warping, DTW) per pair of utterances through the
 * frame-distance matrix of their coder vectors (LLSM_GPU_CODE below), on the device.  It gives the list a morph needs --
 * where, in frames of utterance B, each frame of utterance A belongs -- in the form llsm_gpu_batch_splice takes, and the
 * accumulated cost of the path, which is what unit selection sorts a bank of candidates by.
 * Pair p aligns utterance utt_a[p] of batch a (na frames) with utterance utt_b[p] of batch b (nb frames).  pos is a host
 * array of sum_p na(p) floats, pair after pair in list order; its entries lie in [0, nb - 1], so they go into
 * llsm_gpu_splice_map.pos_b (with utt_b) or .pos_a unchanged.  cost[p] (cost may be NULL) is the accumulated cost of
 * the path of pair p.  Synchronous: on return both arrays are filled.  A refused call returns -1, sets
 * llsm_gpu_last_error() (the message starts with "llsm_gpu_batch_align:"), launches nothing and leaves pos and cost
 * untouched.  The call reads LLSM_GPU_CODE of both batches and writes no array of either; it writes scratch of its own
 * on a only (the distance planes, llsm_gpu_batch_debug_plane(a, 6, ...), always kept); the lowest-F0 bound and every row
 * stay as they were.  a == b is allowed, and an utterance may appear in any number of pairs.
 *
 * The rules, per pair.  A is the [na][dim] rows of a's LLSM_GPU_CODE for the utterance, B likewise.  Everything is
 * float32, one rounding per operation, no contraction.
 *  D1. d = 0; for k = first ... first + count - 1 ascending: t = A[i][k] - B[j][k]; d = d + t * t.  Then D[i][j] =
 *      d + voicing_cost if exactly one of A[i][0], B[j][0] is > 0.5f, else d.  (The squared-difference form, not
 *      |a|^2 + |b|^2 - 2ab: along the path the two frames are close, and the expanded form cancels there.)
 *  D2. acc[0][0] = D[0][0].  Row 0: acc[0][j] = (acc[0][j-1] + step_cost) + D[0][j], move 2.  Column 0: acc[i][0] =
 *      (acc[i-1][0] + step_cost) + D[i][0], move 1.  Elsewhere: m = acc[i-1][j-1], move 0; up = acc[i-1][j] + step_cost, if
 *      up < m: m = up, move 1; lf = acc[i][j-1] + step_cost, if lf < m: m = lf, move 2; acc[i][j] = m + D[i][j].  The moves
 *      on the two borders are forced and not compared, so a NaN in the features cannot send the path outside the matrix.
 *  D3. The path runs from (na - 1, nb - 1) back along the moves (0: i - 1, j - 1; 1: i - 1; 2: j - 1) to (0, 0): at most
 *      na + nb - 2 moves, whatever the bits of LLSM_GPU_CODE.  pos[i] = (float)(lo_i + hi_i) * 0.5f with lo_i and hi_i the
 *      least and the largest j the path visits in row i; cost = acc[na-1][nb-1].
 * A pair's result depends on its own two utterances and the options only: not on the other pairs, their order, the
 * batches around them, or earlier calls.
 *
 * Refused: a NULL batch; n_pairs < 0; different contexts; coder not enabled on either batch, or different coder
 * dimensions; a column range outside [0, dim); a NaN, infinite or negative cost; with n_pairs > 0 a NULL list or pos,
 * an utterance index outside its batch, a named utterance without frames, and a sum of na x nb above 2^28 cells (the
 * message names the total).  n_pairs == 0 returns 0.
 * llsm_gpu_align_check is host only: 0, or -1 with the message llsm_gpu_batch_align would give for these options
 * (NULL: the defaults) on batches whose coder has these orders.
 * Known limits: the whole matrix of a pair is searched, so a call holds pairs of 2^28 cells in all -- long material goes
 * through llsm_gpu_batch_align_band below, which searches a band around the diagonal, or llsm_gpu_batch_align_around, which
 * searches one around the path of a coarser alignment; there are no slope constraints beyond
 * monotonicity -- a path may stay on one frame or skip many: llsm_gpu_batch_align_slope below bounds the local slope. */
typedef struct {
  int     first, count;   /* columns [first, first + count) of LLSM_GPU_CODE are compared; defaults 3 and order_spec
                             (count <= 0: order_spec): the mel-spectrum points */
  FP_TYPE step_cost;      /* added to a move that is not diagonal; default 0; >= 0, finite */
  FP_TYPE voicing_cost;   /* added to a cell whose two frames differ in voicing (code[0] > 0.5f); default 0; >= 0, finite */
} llsm_gpu_align_options;
void llsm_gpu_align_default_options(llsm_gpu_align_options* dst);
int  llsm_gpu_align_check(const llsm_gpu_align_options* opt, int order_spec, int order_bap);
int  llsm_gpu_batch_align(llsm_gpu_batch* a, const llsm_gpu_batch* b, int n_pairs, const int* utt_a, const int* utt_b,
       const llsm_gpu_align_options* opt /* NULL: defaults */, FP_TYPE* pos, FP_TYPE* cost /* may be NULL */);

/* ---- alignment inside a diagonal band: llsm_gpu_batch_align for long utterances.  The path of pair p is searched among
 * the cells within band[p] columns of the straight diagonal only, so the planes, the moves and the time of a pair are
 * na x (2 band + 1) instead of na x nb, and two five-minute renditions (60 000 frames each) under a band of 500 frames are
 * 6e7 cells instead of 3.6e9.  band is a host array of n_pairs half-widths in frames.  The contract is that of
 * llsm_gpu_batch_align -- the same pos and cost, synchronous, a refused call returns -1 with a message that starts with
 * "llsm_gpu_batch_align_band:", launches nothing and leaves pos and cost untouched; LLSM_GPU_CODE of both batches is read and
 * no array of either written; a == b is allowed -- with scratch of its own on a (the band planes,
 * llsm_gpu_batch_debug_plane(a, 9, ...), always kept): the scratch of llsm_gpu_batch_align, plane 6 among it, stays as the
 * last such call left it.  A pair's result depends on its own two utterances, its band and the options only.
 *
 * The rules, per pair; float32, one rounding per operation, no contraction.
 *  B1. The band.  na > 1: c_i = (2 i (nb - 1) + (na - 1)) / (2 (na - 1)) in 64-bit integer division, the diagonal rounded
 *      half up; na == 1: c_0 = 0.  Row i spans the columns lo_i = max(0, c_i - band) ... hi_i = min(nb - 1, c_i + band).
 *      The band is connected when lo_{i+1} <= hi_i + 1 for every i and hi_{na-1} == nb - 1; a connected band contains
 *      (0, 0) and (na - 1, nb - 1), and every cell of it other than (0, 0) has at least one predecessor inside it.
 *      llsm_gpu_align_band_min returns the least connected band (0 for na >= nb with na > 1, nb - 1 for na == 1, 1 for
 *      63 x 64, 31 for 2 x 63), -1 if na < 1 or nb < 1.  llsm_gpu_align_band_rows fills lo and hi (na entries each) and
 *      returns 0, or -1 with a message for na < 1, nb < 1, a NULL array, and a band that is negative or not connected.
 *      Both are host only and need no device.
 *  B2. D[i][j] is rule D1 unchanged, for the cells inside the band only.
 *  B3. acc[0][0] = D[0][0].  Elsewhere the candidates are the predecessors that lie inside the band, in this order:
 *      acc[i-1][j-1], move 0; acc[i-1][j] + step_cost, move 1; acc[i][j-1] + step_cost, move 2.  m starts from the first
 *      candidate that exists, and a later one replaces it only if it is strictly smaller; acc[i][j] = m + D[i][j].  Whether a
 *      predecessor is inside the band is decided by integer comparisons with lo and hi, never by the values, so a NaN or an
 *      infinity in the features cannot send the path outside the band.  Where the band covers the whole matrix this is D2
 *      bit for bit: on row 0 only the left candidate exists, on column 0 only the upper one, elsewhere all three.
 *  B4. D3 unchanged, over the moves of B3: at most na + nb - 2 moves, every cell of the path inside the band;
 *      cost = acc[na-1][nb-1].
 *
 * Refused: everything llsm_gpu_batch_align refuses, and with n_pairs > 0 a NULL band, a negative band, a band that is not
 * connected for its pair (the message names the pair and llsm_gpu_align_band_min of it), and a sum of na x (2 band + 1)
 * above 2^28 cells (the message names the total).  n_pairs == 0 returns 0.
 * Known limits: one wavefront walks a pair; the band follows the straight diagonal and nothing else, so it has to be as
 * wide as the renditions drift apart (llsm_gpu_batch_align_around below searches a band around a line of the caller's
 * instead); there are no slope constraints beyond monotonicity (llsm_gpu_batch_align_slope below has them over the whole
 * matrix, llsm_gpu_batch_align_band_slope inside this band). */
int  llsm_gpu_batch_align_band(llsm_gpu_batch* a, const llsm_gpu_batch* b, int n_pairs, const int* utt_a, const int* utt_b,
       const int* band /* n_pairs half-widths, frames */, const llsm_gpu_align_options* opt /* NULL: defaults */,
       FP_TYPE* pos, FP_TYPE* cost /* may be NULL */);
int  llsm_gpu_align_band_min(int na, int nb);                              /* host only */
int  llsm_gpu_align_band_rows(int na, int nb, int band, int* lo, int* hi);  /* host only; na entries each */

/* ---- slope-constrained alignment: llsm_gpu_batch_align with local slopes in [1/2, 2].  Under rules D2 and B3 a path may
 * stay on one frame of B for any number of frames of A or jump many frames of B inside one row of A -- step_cost only makes
 * that dearer -- and in a morph a stall is a frozen frame, a jump a skipped stretch.  Here every move advances both
 * utterances, by one frame each or by two frames of one and one of the other (Sakoe and Chiba's symmetric step pattern with
 * P = 1).  The contract is that of llsm_gpu_batch_align -- the same pos and cost, the same options and llsm_gpu_align_check,
 * synchronous, a refused call returns -1 with a message that starts with "llsm_gpu_batch_align_slope:", launches and allocates
 * nothing and leaves pos and cost untouched; LLSM_GPU_CODE of both batches is read and no array of either written; a == b is
 * allowed -- with scratch of its own on a (the distance planes, llsm_gpu_batch_debug_plane(a, 12, ...), always kept): planes 6
 * and 9 and the scratch of the other two calls stay as they were.  A pair's result depends on its own two utterances and the
 * options only.
 *
 * The rules, per pair; float32, one rounding per operation, no contraction.
 *  L1. The region.  A pair is admissible when nb - 1 <= 2 (na - 1) and na - 1 <= 2 (nb - 1): 1 x 1 is, 1 x 2 is not.  Row i
 *      holds the columns lo_i = max(ceil(i / 2), (nb - 1) - 2 (na - 1 - i)) ... hi_i = min(2 i, (nb - 1) - ceil((na - 1 - i)
 *      / 2)), integers taken in 64-bit: the cells from which (0, 0) is reached backwards and (na - 1, nb - 1) forwards under
 *      the moves of L3.  lo_i > hi_i is possible (3 x 2: row 1 is (1, 0)): no path stops on such a row, it is only passed
 *      through.  Every cell of the region other than (0, 0) has at least one predecessor of L3 inside the region.
 *      llsm_gpu_align_slope_rows fills lo and hi (na entries each; either may be NULL, both NULL only asks whether the pair
 *      is admissible) and returns 0, or -1 with a message that names na, nb and the bound that fails for na < 1, nb < 1 or a
 *      pair that is not admissible.  Host only, needs no device.
 *  L2. D[i][j] is rule D1 unchanged, for the whole matrix.
 *  L3. acc[0][0] = D[0][0].  For every other cell (i, j) of the region the candidates are, in this order, each only if its
 *      predecessor cell lies in the region (integer comparisons with lo and hi of that row, never of values):
 *        move 0: acc[i-1][j-1];
 *        move 1: (acc[i-2][j-1] + D[i-1][j]) + step_cost;
 *        move 2: (acc[i-1][j-2] + D[i][j-1]) + step_cost.
 *      m starts from the first candidate that exists, and a later one replaces it only if it is strictly smaller;
 *      acc[i][j] = m + D[i][j].  The cell between the two ends of move 1 or 2 need not lie in the region; it is always
 *      inside the matrix.  The additions are in the order of a diagonal move of D2 followed by an upper or a left one, so
 *      every such path is a path of D2 with the same sequence of operations.
 *  L4. The path runs from (na - 1, nb - 1) back along the moves to (0, 0) (0: (i - 1, j - 1); 1: (i - 1, j), then
 *      (i - 2, j - 1); 2: (i, j - 1), then (i - 1, j - 2)): at most min(na, nb) - 1 moves, whatever the bits of
 *      LLSM_GPU_CODE.  pos[i] = (float)(lo + hi) * 0.5f over the least and the largest column visited in row i, the cells in
 *      between included; every row is visited.  cost = acc[na-1][nb-1].  A NaN never replaces a candidate and cannot move the
 *      path out of the region; the cost may then be NaN, as in D2.
 * It follows that pos does not decrease, pos[i+1] - pos[i] <= 2, pos[i+2] - pos[i] >= 1, a row spans at most two columns,
 * and, for finite features, cost is never below the cost of llsm_gpu_batch_align on the same pair as float32 values
 * (rounded addition and minimum are monotone, and the paths are a subset with the same order of operations).
 *
 * Refused: everything llsm_gpu_batch_align refuses, by the same code and in the same order, the cap of 2^28 cells on the sum
 * of na x nb among it; and with n_pairs > 0 a pair that is not admissible (the message names the pair, na and nb), checked
 * pair by pair before anything is allocated.  n_pairs == 0 returns 0.
 * Known limits: the whole matrix of D is computed although the region is about a third of a square pair, so the cap holds a
 * pair to about 16 400 x 16 400 -- longer material goes through llsm_gpu_batch_align_band_slope below, the same pattern inside
 * a band, or llsm_gpu_batch_align_around with slope = 1, inside a band around a line; one wavefront walks a pair; P = 1 is the
 * only pattern. */
int  llsm_gpu_align_slope_rows(int na, int nb, int* lo, int* hi);   /* host only; lo, hi: na entries each, both may be NULL */
int  llsm_gpu_batch_align_slope(llsm_gpu_batch* a, const llsm_gpu_batch* b, int n_pairs, const int* utt_a, const int* utt_b,
       const llsm_gpu_align_options* opt /* NULL: defaults */, FP_TYPE* pos, FP_TYPE* cost /* may be NULL */);

/* ---- slope-constrained alignment inside a diagonal band: the moves of llsm_gpu_batch_align_slope searched among the cells
 * of the band of llsm_gpu_batch_align_band, so that long material -- two five-minute renditions of 60 000 frames under a band of
 * 500 -- gets a path without stalls and jumps: the planes, the moves and the time of a pair are na x (2 band + 1).  The contract
 * is that of llsm_gpu_batch_align_band -- the same band array, the same pos and cost, the same options and
 * llsm_gpu_align_check, synchronous, a refused call returns -1 with a message that starts with
 * "llsm_gpu_batch_align_band_slope:", launches and allocates nothing and leaves pos and cost untouched; LLSM_GPU_CODE of both
 * batches is read and no array of either written; a == b is allowed -- with scratch of its own on a (the band planes,
 * llsm_gpu_batch_debug_plane(a, 13, ...), always kept): planes 6, 9 and 12 and the scratch of the other three calls stay as they
 * were.  A pair's result depends on its own two utterances, its band and the options only.
 *
 * The rules, per pair; float32, one rounding per operation, no contraction; integers taken in 64 bits.
 *  K1. The region.  A pair must be admissible under L1.  p_i ... q_i is the column range of row i of the band of rule B1
 *      (lo_i and hi_i there, c_i unchanged).  A move of L3 is allowed when both of its ends lie in the band and the cell it
 *      passes lies in the band: move 1 passes (i - 1, j), move 2 passes (i, j - 1).  The region is the set of cells that lie on
 *      some path of allowed moves from (0, 0) to (na - 1, nb - 1).  It is computed by two integer sweeps over intervals; an
 *      interval with lower end > upper end is empty, and empty intervals contribute nothing.
 *        Forward.  F_0 = [0, 0].  For i >= 1, with F_{i-1} = [a, b] and F_{i-2} = [c, d], the pieces are
 *          [max(a + 1, p_i), min(b + 1, q_i)] for move 0, [max(a + 2, p_i + 1), min(b + 2, q_i)] for move 2 and, for i >= 2,
 *          [max(c + 1, p_i, p_{i-1}), min(d + 1, q_i, q_{i-1})] for move 1; F_i runs from the least lower end to the largest
 *          upper end of the non-empty pieces.
 *        Backward.  G_{na-1} = [nb - 1, nb - 1] if q_{na-1} >= nb - 1, else empty.  For i < na - 1, with G_{i+1} = [a, b] and
 *          G_{i+2} = [c, d], the pieces are [max(a - 1, p_i), min(b - 1, q_i)], [max(a - 2, p_i, p_{i+1} - 1), min(b - 2, q_i)]
 *          and, for i + 2 < na, [max(c - 1, p_i, p_{i+1} - 1), min(d - 1, q_i, q_{i+1} - 1)].
 *      Row i of the region is the intersection of F_i and G_i; an empty row is reported as lo = 1, hi = 0: no path stops on
 *      it, it is only passed through, as in L1.  The band is connected for the slope pattern when row na - 1 is non-empty; it
 *      is then [nb - 1, nb - 1], and row 0 is [0, 0].  Connectedness is monotone in band.
 *      That the pieces always join into one interval -- so that the sweeps give exactly the reachable sets --, that lo and
 *      hi of a connected band do not decrease over the non-empty rows and that no two consecutive rows are empty is MEASURED,
 *      not proven: the rule rests on tests/test_align_band_slope_host.py, which compares the sweeps with reachability cell
 *      by cell for every admissible na, nb <= 40 at every band.  With band >= nb - 1 the non-empty rows are those of L1; the
 *      least connected band is 0 or 1 for every admissible pair up to 70 x 70 (64 x 64: 0; 63 x 64: 1).
 *      llsm_gpu_align_band_slope_min returns the least connected band, or -1 with a message for na < 1, nb < 1, a pair that
 *      is not admissible or na above 2^28 (the sweeps hold a few words per row, and no call takes such a pair).
 *      llsm_gpu_align_band_slope_rows fills lo and hi (na entries each; either may be NULL, both NULL only asks whether the
 *      band is connected) and returns 0, or -1 with a message that names na, nb and the band -- and
 *      llsm_gpu_align_band_slope_min of the pair where the band is not connected -- for na < 1, nb < 1, a pair that is not
 *      admissible, na above 2^28, and a band that is negative or not connected for the pattern.  Both are host only and
 *      need no device.
 *  K2. D[i][j] is rule D1 unchanged, for the cells of the band only (rule B2 unchanged).
 *  K3. acc[0][0] = D[0][0].  For every other cell (i, j) of the region the candidates are, in this order:
 *        move 0: acc[i-1][j-1], if (i - 1, j - 1) is in the region;
 *        move 1: (acc[i-2][j-1] + D[i-1][j]) + step_cost, if (i - 2, j - 1) is in the region and p_{i-1} <= j <= q_{i-1};
 *        move 2: (acc[i-1][j-2] + D[i][j-1]) + step_cost, if (i - 1, j - 2) is in the region and j - 1 >= p_i.
 *      m starts from the first candidate that exists, and a later one replaces it only if it is strictly smaller;
 *      acc[i][j] = m + D[i][j].  Which candidates exist is decided by integer comparisons with the rows of the region and of
 *      the band, never by values.  Every cell of the region other than (0, 0) has a candidate.
 *  K4. L4 unchanged, over the moves of K3: at most min(na, nb) - 1 moves; pos[i] from the least and the largest column visited
 *      in row i, the passed cells included; every row is visited; cost = acc[na-1][nb-1].  A NaN never replaces a candidate
 *      and cannot move the path out of the region.
 * It follows that the properties of pos listed under L4 hold, and every pos[i] lies in [p_i, q_i]; that where the band covers
 * the matrix (band >= nb - 1) pos and cost are the bits of llsm_gpu_batch_align_slope; and that, for finite features, cost is
 * never below the cost of llsm_gpu_batch_align_slope on the pair, nor below that of llsm_gpu_batch_align_band with the same
 * band: each path here is a path of those rules with the same sequence of operations.
 *
 * Refused: everything llsm_gpu_batch_align refuses, by the same code and in the same order; and with n_pairs > 0 a NULL band,
 * a negative band, a pair that is not admissible under L1 (in the words of llsm_gpu_batch_align_slope), a band that is not
 * connected for the slope pattern on its pair (the message names the pair and llsm_gpu_align_band_slope_min of it), and a sum
 * of na x (2 band + 1) above 2^28 cells (the message names the total).  n_pairs == 0 returns 0.
 * Known limits: one wavefront walks a pair; the band follows the straight diagonal and nothing else
 * (llsm_gpu_batch_align_around below, with slope = 1, follows a line of the caller's); P = 1 is the only pattern; the rows
 * of the region are computed on the host, na steps per pair and call. */
int  llsm_gpu_batch_align_band_slope(llsm_gpu_batch* a, const llsm_gpu_batch* b, int n_pairs, const int* utt_a, const int* utt_b,
       const int* band /* n_pairs half-widths, frames */, const llsm_gpu_align_options* opt /* NULL: defaults */,
       FP_TYPE* pos, FP_TYPE* cost /* may be NULL */);
int  llsm_gpu_align_band_slope_min(int na, int nb);                                  /* host only */
int  llsm_gpu_align_band_slope_rows(int na, int nb, int band, int* lo, int* hi);     /* host only; na entries each, both may be NULL */

/* ---- alignment inside a band that follows a centre line: the two banded calls above search around the straight diagonal
 * and nothing else, which holds them to takes recorded against a click -- two freely spoken renditions of five minutes
 * drift apart by seconds, and the band that holds the drift passes the cap or costs what the whole matrix would.  Here the
 * caller gives the column c_i around which row i is searched, so that alignment can go from coarse to fine: align a
 * coarse copy of the pair with llsm_gpu_batch_align_slope (the pooled vectors of llsm_gpu_batch_pool_code uploaded to a small
 * batch, or llsm_gpu_batch_retime + llsm_gpu_batch_encode), turn its pos into a line with llsm_gpu_align_center_line, and
 * search the fine pair within a few times the pooling factor of it.  llsm_gpu_batch_align_pyramid below runs exactly these
 * steps in one call, with the pooled vectors kept on the device, and picks a connected band itself.  center is a host array of sum_p na(p) columns, pair after pair in
 * list order (the layout of pos); band one half-width per pair; slope chooses the moves: 0 those of
 * llsm_gpu_batch_align_band, 1 those of llsm_gpu_batch_align_band_slope.  The contract is that of llsm_gpu_batch_align_band --
 * the same pos and cost, the same options and llsm_gpu_align_check, synchronous, a refused call returns -1 with a message that
 * starts with "llsm_gpu_batch_align_around:", launches and allocates nothing and leaves pos and cost untouched;
 * LLSM_GPU_CODE of both batches is read and no array of either written; a == b is allowed; an utterance may appear in any
 * number of pairs, each with a line of its own -- with one scratch set of its own on a for both values of slope (the band
 * planes, llsm_gpu_batch_debug_plane(a, 14, ...), always kept): planes 6, 9, 12 and 13 and the scratch of the four other calls
 * stay as they were.  A pair's result depends on its own two utterances, its line, its band, slope and the options only.
 *
 * The rules, per pair; float32, one rounding per operation, no contraction; integers taken in 64 bits.
 *  A1. The line and the band.  c_i = center[pos0 + i], pos0 being the pair's offset into pos.  A line is valid when
 *      0 <= c_i <= nb - 1 for every i and c_{i+1} >= c_i.  Row i spans the columns p_i = max(0, c_i - band) ...
 *      q_i = min(nb - 1, c_i + band).
 *      slope = 0: the band is connected when p_0 == 0, q_{na-1} == nb - 1 and p_{i+1} <= q_i + 1 for every i; then every cell
 *      of it other than (0, 0) has a predecessor of B3 inside it.  The least connected band is max(c_0, nb - 1 - c_{na-1},
 *      max_i (c_{i+1} - c_i) / 2) in integer division (na == 1: max(c_0, nb - 1 - c_0)).
 *      slope = 1: the pair must be admissible under L1.  The region is that of the two interval sweeps of K1 over these p and
 *      q: F_0 = [0, 0] if p_0 <= 0, else empty, and the rest is K1 word for word -- the forward pieces, G_{na-1} = [nb - 1,
 *      nb - 1] if q_{na-1} >= nb - 1, the backward pieces, row i the intersection of F_i and G_i, an empty row (1, 0).  The
 *      band is connected when row na - 1 of the region is non-empty.  Connectedness is monotone in band, and the band that
 *      covers the matrix (band >= nb - 1) is connected for an admissible pair: its region is that of L1.
 *      That the pieces of a row join into one interval for any line -- so that the sweeps give exactly the cells that lie on
 *      a path of allowed moves --, that no two consecutive rows of a connected region are empty and that lo and hi do not
 *      decrease over its non-empty rows under a non-decreasing line is MEASURED by tests/test_align_around_host.py, which
 *      compares the sweeps with reachability cell by cell under straight and under random lines.  The reason the pieces
 *      touch: move 0 from a cell of row i - 2 lands inside F_{i-1}, one column left of where move 1 from the same cell lands
 *      in row i, so the piece of move 1 is never apart from those of moves 0 and 2 out of F_{i-1}.
 *      llsm_gpu_align_around_rows fills lo and hi (na entries each; either may be NULL, both NULL only asks whether the band
 *      is connected): for slope = 0 the band's rows p, q, for slope = 1 the region's rows with an empty row as (1, 0).  It
 *      returns 0, or -1 with a message for na < 1, nb < 1, na above 2^28, a slope that is neither 0 nor 1, a NULL line,
 *      under slope = 1 a pair that is not admissible (the message names na, nb and the bound), a line that is not valid
 *      (the message names the row and its value), a negative band, and a band that is not connected (the message names
 *      the band, na, nb and llsm_gpu_align_around_min of the line).  llsm_gpu_align_around_min returns the least connected
 *      band -- for slope = 0 the closed form above, for slope = 1 by bisection over [0, nb - 1] --, or -1 with a message
 *      for what _around_rows refuses before it looks at the band.
 *      llsm_gpu_align_center_line turns pos_c of an alignment of a coarse pair of na_c x nb_c frames into a line for the
 *      fine pair of na x nb.  In float64, one rounding per operation: x = (i (na_c - 1)) / (na - 1), k = min(floor(x),
 *      na_c - 2), y = pos_c[k] + (pos_c[k+1] - pos_c[k]) (x - k) -- y = pos_c[0] where na_c == 1 or na == 1 --,
 *      s = (nb - 1) / (nb_c - 1), or 0 where nb_c == 1, c_i = min(nb - 1, max(0, floor(y s + 0.5))), and then a running
 *      maximum, so that the line does not decrease.  The result is always a valid line; the band remains the caller's
 *      choice, with llsm_gpu_align_around_min as the floor.  Returns 0, or -1 with a message for a size below 1, a NULL array
 *      and an entry of pos_c that is NaN or outside [0, nb_c - 1] (the message names the entry and its value).
 *      The three are host only and need no device.
 *  A2. D[i][j] is rule D1 unchanged, for the cells of the band only (rule B2), in the layout of plane 14.
 *  A3. slope = 0: rules B3 - B4 over these rows.  slope = 1: rules K3 - K4 over this region and this band.
 * It follows, and tests/test_gpu_align_around.py holds it to the bit, that with center the diagonal of B1 pos, cost and plane 14
 * are those of llsm_gpu_batch_align_band and its plane 9 (slope = 0) or of llsm_gpu_batch_align_band_slope and its plane 13
 * (slope = 1); that with band >= nb - 1 and any valid line pos and cost are those of llsm_gpu_batch_align or
 * llsm_gpu_batch_align_slope; and that for finite features cost is never below the cost of that full call.
 *
 * Refused, each check over all pairs before the next, before anything is allocated, copied or launched: (1) everything
 * llsm_gpu_batch_align refuses short of its cap, by the same code and in the same order; (2) a slope that is neither 0 nor 1;
 * with n_pairs > 0 (3) a NULL band or center, (4) a negative band, (5) under slope = 1 a pair that is not admissible under L1,
 * in the words of llsm_gpu_batch_align_slope, (6) a line that is not valid (the message names the pair, the row and the
 * value), (7) a band that is not connected (the message names the pair and llsm_gpu_align_around_min of it), and (8) a sum of
 * na x (2 band + 1) above 2^28 cells (the message names the total).  n_pairs == 0 returns 0.
 * Known limits: one wavefront walks a pair; the coarse pass is the caller's here -- llsm_gpu_batch_align_pyramid below runs
 * both; under a line that climbs
 * by whole bands per row the distance tiles of a strip of 64 rows cover far more cells than the band holds. */
int  llsm_gpu_batch_align_around(llsm_gpu_batch* a, const llsm_gpu_batch* b, int n_pairs, const int* utt_a, const int* utt_b,
       const int* center /* sum_p na(p) columns, pair after pair in list order: the layout of pos */,
       const int* band   /* n_pairs half-widths, frames */,
       int slope         /* 0: the moves of llsm_gpu_batch_align_band; 1: those of llsm_gpu_batch_align_band_slope */,
       const llsm_gpu_align_options* opt /* NULL: defaults */, FP_TYPE* pos, FP_TYPE* cost /* may be NULL */);
int  llsm_gpu_align_around_rows(int na, int nb, const int* center, int band, int slope, int* lo, int* hi);  /* host only */
int  llsm_gpu_align_around_min(int na, int nb, const int* center, int slope);                               /* host only */
int  llsm_gpu_align_center_line(int na_c, int nb_c, const FP_TYPE* pos_c, int na, int nb, int* center);     /* host only */

/* ---- pooled coder vectors: the mean of every `factor` consecutive rows of LLSM_GPU_CODE of an utterance, computed on the
 * device -- the input of a coarse alignment.  A mean and not every factor-th row: a decimated track aliases (a plosive of
 * two frames is there or not by the phase of the grid), the mean of a group is a low-pass before the decimation and sees
 * every frame.
 *  P1. For an utterance of n frames and a factor f in [1, 64] there are nc = (n + f - 1) / f coarse frames
 *      (llsm_gpu_pool_frames: nc, or -1 with a message for nfrm < 1 or a factor outside the range; host only).  Coarse frame k
 *      pools the frames j = k f ... min(n, (k + 1) f) - 1, m of them -- the last group of an utterance may be short.  For
 *      every column c of LLSM_GPU_CODE, the voicing column 0 included: s = 0.0f; for j ascending: s = s + CODE[j][c];
 *      out[k][c] = s / (float)m.  float32, one rounding per operation, the division correctly rounded; the order of the
 *      additions is part of the rule.  Pooled column 0 is the voiced share of the group, which rule D1's > 0.5f reads as a
 *      majority vote.  factor == 1 copies the rows, except that -0.0f becomes +0.0f.  A NaN or an infinity in a group
 *      spreads to its mean in that column and no further.
 * llsm_gpu_batch_pool_code pools the n utterances named in utts (repeats allowed, any order) and writes them to the host
 * array dst one after another in list order, each [nc][dim] row-major.  Synchronous.  It reads LLSM_GPU_CODE and writes no
 * array and no scratch of the batch.  Refused with -1, a message that starts with "llsm_gpu_batch_pool_code:", nothing
 * launched and dst untouched: a NULL batch; a coder that is not enabled; a factor outside [1, 64]; n < 0; with n > 0 a NULL
 * list or dst, an index outside the batch, an utterance without frames, and a total above 2^28 coarse frames.  n == 0
 * returns 0. */
int  llsm_gpu_pool_frames(int nfrm, int factor);                       /* host only */
int  llsm_gpu_batch_pool_code(const llsm_gpu_batch* b, int factor, int n, const int* utts, FP_TYPE* dst);

/* ---- coarse-to-fine alignment in one call: the recipe above llsm_gpu_batch_align_around -- pool, align the coarse pair,
 * turn its positions into a line, pick a band, search the fine pair around the line -- for every pair of a list, with the
 * pooled vectors formed and kept on the device: LLSM_GPU_CODE does not cross the link, no throw-away batch is made, and
 * the band is chosen so that it is connected.  pos and cost are those of llsm_gpu_batch_align_around under the line and the
 * band the call made; center_out (sum_p na(p) columns, the layout of pos; may be NULL) receives the lines and band_out
 * (n_pairs; may be NULL) the bands.  Synchronous.  A refused call returns -1 with a message that starts with
 * "llsm_gpu_batch_align_pyramid:" and leaves pos, cost, center_out and band_out untouched.  LLSM_GPU_CODE of both batches is
 * read and no array of either written; a == b is allowed, and an utterance may appear in any number of pairs.  A pair's
 * result depends on its own two utterances, factor, margin, slope and the options only.  Scratch: two sets of its own on a,
 * one per pass, the pooled vectors among them; planes 6, 9, 12, 13 and 14 and the scratch of the five calls above stay as
 * they were, and the two sets have no plane number in llsm_gpu_batch_debug_plane.
 *
 * The rules, per pair of na x nb frames.
 *  Y1. Both utterances are pooled by P1 to nca x ncb vectors.
 *  Y2. The pooled pair is aligned with opt unchanged: slope = 0 by rules D1 - D3 of llsm_gpu_batch_align, slope = 1 by rules
 *      L1 - L4 of llsm_gpu_batch_align_slope.  This gives pos_c[0 .. nca).
 *  Y3. center = llsm_gpu_align_center_line(nca, ncb, pos_c, na, nb): that function, not a restatement of it.
 *  Y4. band = max(min(margin x factor, nb - 1), llsm_gpu_align_around_min(na, nb, center, slope)), the product taken in 64
 *      bits: margin is the half-width in coarse frames, and the band is always connected.
 *  Y5. Rules A1 - A3 of llsm_gpu_batch_align_around with this line, this band and slope.
 * It follows, and tests/test_gpu_align_pyramid.py holds it to the bit, that the call gives what llsm_gpu_batch_pool_code,
 * llsm_gpu_batch_align or _slope on batches that hold the pooled vectors, llsm_gpu_align_center_line,
 * llsm_gpu_align_around_min and llsm_gpu_batch_align_around give when run by hand; that with margin x factor >= nb - 1 pos
 * and cost are those of llsm_gpu_batch_align (slope = 0) or llsm_gpu_batch_align_slope (slope = 1) on the fine pair; and that
 * for finite features cost is never below the cost of that full call.  A 1 x 1 coarse pair (both utterances no longer than
 * factor) gives an all-zero line, which llsm_gpu_align_around_min answers with nb - 1: the whole matrix.
 *
 * Refused, each check over all pairs before the next, before anything is allocated, copied or launched: (1) everything
 * llsm_gpu_batch_align refuses short of its cap, by the same code and in the same order (n_pairs == 0 returns 0 here, as it
 * does there); (2) a factor outside [2, 64], a negative margin, a slope that is neither 0 nor 1; (3) under slope = 1 a fine
 * pair that is not admissible under L1, in the words of llsm_gpu_batch_align_slope, or a coarse pair that is not (the message
 * names the pair, both sizes and the factor: 64 x 127 frames pool to 1 x 2 at factor 64 -- a smaller factor is the remedy);
 * (4) a sum of nca x ncb above 2^28 cells.  The cap of the fine pass, a sum of na x (2 band + 1) above 2^28 cells, is known
 * only after the coarse pass: it is refused then, in the words of llsm_gpu_batch_align_around, with pos, cost, center_out and
 * band_out untouched -- but the call's own coarse scratch and pooled vectors have been written by then (nothing a caller can
 * observe: they have no plane).
 * Known limits: one wavefront walks a pair in either pass; two levels only; an utterance that appears in k pairs is pooled
 * k times; the lines and the bands are made on the host between the passes, na steps per pair (times log2 nb under
 * slope = 1, whose least band is found by bisection). */
int  llsm_gpu_batch_align_pyramid(llsm_gpu_batch* a, const llsm_gpu_batch* b, int n_pairs, const int* utt_a, const int* utt_b,
       int factor   /* 2 .. 64 */,
       int margin   /* >= 0, half-width of the fine band in COARSE frames */,
       int slope    /* 0 or 1, as llsm_gpu_batch_align_around */,
       const llsm_gpu_align_options* opt /* NULL: defaults */,
       FP_TYPE* pos, FP_TYPE* cost /* may be NULL */,
       int* center_out /* sum_p na(p), layout of pos; may be NULL */,
       int* band_out   /* n_pairs; may be NULL */);

/* ---- open-ended (subsequence) alignment: a query inside a take.  Every call above forces its path through both corners of
 * the matrix, which is right for two trimmed renditions of one phrase and wrong for a phrase that lies somewhere in a long
 * take, or for two takes whose leading and trailing silences differ.  Here pair p aligns the WHOLE of utterance utt_a[p] of
 * a, the query of na frames, with SOME stretch of utterance utt_b[p] of b, the take of nb frames: the path may start on any
 * column of row 0 and end on any column of the last row, at no cost.  The call gives where the query lies in the take
 * (span), the path through it in the form llsm_gpu_batch_splice takes (pos), its cost, and the matching function along the
 * take (last_row), from which a caller finds further occurrences.
 * pos is sum_p na(p) floats as in llsm_gpu_batch_align; all entries of a pair lie in [begin, end] within [0, nb - 1], so they
 * go into llsm_gpu_splice_map.pos_a or .pos_b with utt_b unchanged.  span (2 n_pairs ints; may be NULL): span[2 p] = begin
 * and span[2 p + 1] = end, the first and the last frame of the take on the path, exact integers that never pass through a
 * float (nb may exceed 2^24).  cost[p] (may be NULL) is the accumulated cost at the end.  last_row (sum_p nb(p) floats, pair
 * after pair; may be NULL) is acc of the query's last row along the take.  The contract is that of llsm_gpu_batch_align --
 * the same options and llsm_gpu_align_check, synchronous, a == b allowed, LLSM_GPU_CODE of both batches read and no array of
 * either written, the lowest-F0 bound as it was; a refused call returns -1 with a message that starts with
 * "llsm_gpu_batch_align_sub:", launches and allocates nothing and leaves all four outputs untouched.  The scratch set is the
 * call's own, on a: planes 6, 9, 12, 13 and 14 and the scratch of every call above stay as they were.  A pair's result depends
 * on its own two utterances, slope and the options only.
 *
 * The rules, per pair; float32, one rounding per operation, no contraction.
 *  Q1. The region.  slope = 0: every cell; every pair with na, nb >= 1 is admissible.  slope = 1: row i holds the columns
 *      lo_i = ceil(i / 2) ... hi_i = nb - 1, integers taken in 64-bit: the cells reached from some cell of row 0 under the
 *      moves of L3; a pair is admissible when ceil((na - 1) / 2) <= nb - 1.  There is no upper cut: any cell of the last row
 *      may end a path, and a cell that cannot reach the last row is computed and never lies on the path.  Every cell of the
 *      region below row 0 has a predecessor inside it.  llsm_gpu_align_sub_rows fills lo and hi (na entries each; either
 *      may be NULL, both NULL only asks whether the pair is admissible) and returns 0, or -1 with a message that names na, nb
 *      and the bound that fails for na < 1, nb < 1, a slope that is neither 0 nor 1 or a pair that is not admissible.  Host
 *      only, needs no device.
 *  Q2. D[i][j] is rule D1 unchanged, for the whole matrix.
 *  Q3. acc[0][j] = D[0][j] for every j of row 0: a path may start anywhere on it at no cost, and row 0 has no moves.  For
 *      i >= 1 with slope = 0, D2 unchanged: column 0 is forced, acc[i][0] = (acc[i-1][0] + step_cost) + D[i][0], move 1;
 *      elsewhere the diagonal comes first, then up, then left, and a later candidate replaces an earlier one only if it is
 *      strictly smaller.  For i >= 1 with slope = 1, L3 unchanged over the region of Q1: a candidate exists only if its
 *      predecessor cell lies in the region, which is decided by integer comparisons, never by values.
 *  Q4. end is found by walking the last row's range with j ascending: it starts on lo_{na-1} and is replaced only by a
 *      column whose acc is strictly smaller -- the smallest column of least acc; a NaN never replaces a candidate.
 *      cost = acc[na-1][end].  last_row[j] = acc[na-1][j] inside the row's range, +infinity for j < lo_{na-1}.
 *  Q5. The path runs from (na - 1, end) back along the moves until it reaches row 0; begin is its column there: at most
 *      na - 1 + end moves, whatever the bits of LLSM_GPU_CODE.  pos follows D3 (slope = 0) or L4 (slope = 1), the cells
 *      between the two ends of a move included.  The path stays inside the matrix under NaN, as in D2 and L3.
 * It follows, and tests/test_align_sub_host.py and tests/test_gpu_align_sub.py hold it, that pos[0] == begin; that for finite
 * features and slope = 0 pos[na - 1] == end (a left move into the end cell would make its left neighbour no larger); that
 * for slope = 1 pos[na - 1] is end or end - 0.5 and pos obeys the step bounds of L4; and that for finite features cost is
 * never above the cost of llsm_gpu_batch_align on the same pair as float32 values -- with slope = 1 that of
 * llsm_gpu_batch_align_slope, where that call admits the pair: every acc here is <= the acc there by induction, as rounded
 * addition and minimum are monotone, and the end is a minimum over a row that contains the corner.
 *
 * Refused, every check before anything is allocated: everything llsm_gpu_batch_align refuses, by the same code and in the
 * same order, the cap of 2^28 cells on the sum of na x nb among it; then a slope that is neither 0 nor 1; then, with
 * slope = 1, a pair that is not admissible (the message names the pair, na and nb).  n_pairs == 0 returns 0.
 * llsm_gpu_batch_align_sub_plane returns the distance planes of the last successful llsm_gpu_batch_align_sub with a as a,
 * pair after pair, each [na][nb], laid out as plane 12 of llsm_gpu_batch_debug_plane: the number of floats, with dst == NULL
 * the size only, -1 with a message for a destination of fewer than that many floats (cap) and until such a call has run.  It
 * is a call of its own: the planes have no number in llsm_gpu_batch_debug_plane.
 * Known limits: one wavefront walks a pair; the whole matrix is computed, so the cap holds a 200-frame query to a take of
 * 1.3 million frames in all; there is no band; one occurrence is returned per pair -- last_row is there for the others. */
int  llsm_gpu_align_sub_rows(int na, int nb, int slope, int* lo, int* hi);   /* host only; na entries each, both may be NULL */
int  llsm_gpu_batch_align_sub(llsm_gpu_batch* a, const llsm_gpu_batch* b, int n_pairs, const int* utt_a, const int* utt_b,
       int slope, const llsm_gpu_align_options* opt /* NULL: defaults */, FP_TYPE* pos,
       int* span /* 2 n_pairs: begin, end of each pair; may be NULL */, FP_TYPE* cost /* may be NULL */,
       FP_TYPE* last_row /* sum of nb floats, pair after pair; may be NULL */);
long long llsm_gpu_batch_align_sub_plane(llsm_gpu_batch* a, float* dst, long long cap);

/* ---- unit selection: for every frame of a target batch the frame of a bank that renders it, on the device.  A frame-level
 * search -- the K = 8 nearest bank frames of every target frame under the distance of llsm_gpu_batch_align, from anywhere
 * in the bank -- and then one minimum-cost path per target utterance through these candidates, with a join cost between
 * the choices of neighbouring frames that is zero where the bank simply continues.  It gives the index lists
 * llsm_gpu_batch_splice renders, so that encode -> select -> splice -> tolayer0 -> synthesize stays on the device.
 * utt and pos are host arrays of t.total_frames entries in t's flat frame order: utt[g] is the bank utterance and pos[g]
 * the frame within it, as a float, of the bank frame chosen for target frame g.  They go into llsm_gpu_splice_map.utt_a /
 * .pos_a unchanged (dst shaped like t, src = bank), or into the _b side.  cost[u] (cost may be NULL; n_utt entries of t)
 * is the accumulated cost of the path of utterance u, 0 for an utterance without frames.  Synchronous: on return the
 * arrays are filled.  A refused call returns -1, sets llsm_gpu_last_error() (the message starts with
 * "llsm_gpu_batch_select:"), launches nothing and leaves the three arrays untouched.  The call reads LLSM_GPU_CODE of both
 * batches and writes no array of either; it writes scratch of its own on t only (planes 7 and 8 of
 * llsm_gpu_batch_debug_plane among it); the lowest-F0 bound and every row stay as they were.  t == bank is allowed.
 *
 * The rules.  T is the [t.total_frames][dim] rows of t's LLSM_GPU_CODE, B the rows of the bank's, f a flat frame index
 * of the bank in its frame order.  Everything is float32, one rounding per operation, no contraction.
 *  S1. d(x, y) is rule D1 above between the rows x and y: d = 0; for k = first ... first + count - 1 ascending:
 *      t = x[k] - y[k]; d = d + t * t; then d + voicing_cost if exactly one of x[0], y[0] is > 0.5f.  c(x, y) = d if
 *      d < 1e30f (a float32 comparison), else 1e30f: a NaN or infinite distance becomes 1e30f.  Nothing from here on can
 *      produce a NaN: every term is >= 0 and finite or +infinity, there is no subtraction, and no product of 0 with an
 *      infinity (c is finite).  An infinity is possible only where the options are that large: join_weight * c and
 *      join_cost + ... overflow float32 above about 3.4e38 (join_weight 1e30 on c = 1e30, say), and so may a long sum of
 *      such terms.  Infinite costs compare and tie like any others under S4, and every index stays in the bank.
 *  S2. Every bank frame is eligible for target frame g of utterance u; with skip_own_utterance the frames of bank
 *      utterance u are not.  The K = 8 eligible frames that are lowest under the total order (c(T[g], B[f]), f)
 *      ascending are kept, in that order; n_u = min(8, eligible frames) is the same for every frame of u.  Plane 7,
 *      [t.total_frames][16]: row g holds c[0..7] and then the frame indices as floats; slots >= n_u hold 1e30f and -1.
 *      The order is total, so the result does not depend on how the bank is cut among workgroups.
 *  S3. For frame i >= 1 of an utterance, slot a of frame i - 1 (bank frame fa) and slot j of frame i (bank frame fb):
 *      if fb == fa + 1 and both lie in one bank utterance, J = 0 (a natural continuation).  Otherwise s = fa + 1 if that
 *      frame lies in fa's utterance, else fa, and J = join_cost + join_weight * c(B[s], B[fb]): one multiplication, then
 *      one addition.  Plane 8, [t.total_frames][64]: entry 8 a + j; the rows of first frames and the entries of absent
 *      slots are 0.
 *  S4. States are the slots 0 ... n_u - 1; an absent slot is never a predecessor or an end state.  acc_0[j] = c_0[j].
 *      For i >= 1: m is found over a ascending, starting with acc_{i-1}[0] + J(0, j) and replaced only by a strictly
 *      smaller acc_{i-1}[a] + J(a, j); the back pointer is that a; acc_i[j] = m + c_i[j].  No per-frame normalisation.
 *      The path ends in the smallest state of least acc on the last frame and follows the back pointers; cost[u] is
 *      that acc.
 *  S5. utt[g] is the bank utterance of the chosen slot's bank frame and pos[g] = (float)(its frame within that utterance).
 * A target utterance's result depends on its own rows, the bank and the options only: not on the other target
 * utterances, its place in t, or earlier calls.
 *
 * Refused, before anything is allocated or launched: a NULL batch; different contexts; coder not enabled on either batch,
 * or different coder dimensions; a column range outside [0, dim); a NaN, infinite or negative cost or weight;
 * skip_own_utterance not 0 or 1, or 1 with t != bank; with target frames present a NULL utt or pos, a bank without
 * frames, a bank of more than 2^24 frames (plane 7 keeps indices as floats), and skip_own_utterance leaving a target
 * utterance that has frames without an eligible bank frame.  A t without frames returns 0.
 * llsm_gpu_select_check is host only: 0, or -1 with the message llsm_gpu_batch_select would give for these options
 * (NULL: the defaults) on batches whose coder has these orders.
 * Known limits: the candidates are the eight nearest frames only; llsm_gpu_batch_select_chain below adds the successors of
 * the previous frame's candidates.  The search is exact and exhaustive: there is no index, and no matrix-core form, because the squared-difference rule has two roundings per term. */
typedef struct {
  int     first, count;        /* columns [first, first + count) of LLSM_GPU_CODE are compared; defaults 3 and order_spec
                                  (count <= 0: order_spec) */
  FP_TYPE voicing_cost;        /* as llsm_gpu_align_options; default 0; >= 0, finite */
  FP_TYPE join_cost;           /* added to every transition that is not a natural continuation; default 0; >= 0, finite */
  FP_TYPE join_weight;         /* weight of the spectral join distance; default 1; >= 0, finite */
  int     skip_own_utterance;  /* 1: with t == bank, frames of the target's own utterance are not candidates; default 0 */
} llsm_gpu_select_options;
void llsm_gpu_select_default_options(llsm_gpu_select_options* dst);
int  llsm_gpu_select_check(const llsm_gpu_select_options* opt, int order_spec, int order_bap);
int  llsm_gpu_batch_select(llsm_gpu_batch* t, const llsm_gpu_batch* bank, const llsm_gpu_select_options* opt /* NULL: defaults */,
       int* utt, FP_TYPE* pos, FP_TYPE* cost /* may be NULL */);

/* ---- chained unit selection: llsm_gpu_batch_select with the continuations of the previous frame's states added to the
 * candidates of every frame.  Where the bank holds several similar renditions the frame after the one just chosen is
 * often ninth or tenth nearest: llsm_gpu_batch_select then has to jump to another utterance and pay a join, and the
 * rendered note hops between recordings; here the continuation is a candidate because its predecessor was one.
 * The contract is that of llsm_gpu_batch_select word for word: synchronous; utt, pos and cost have the same form and go
 * into llsm_gpu_splice_map unchanged; t == bank is allowed and skip_own_utterance works as it does there; only
 * LLSM_GPU_CODE of both batches is read and no array of either is written; a t without frames returns 0 with every cost 0;
 * a refused call returns -1, launches nothing, allocates nothing and leaves the three arrays untouched.  The refusals are
 * those listed above, by the same code; every message starts with "llsm_gpu_batch_select_chain:".  llsm_gpu_select_check,
 * llsm_gpu_select_default_options and the options struct serve both calls.  The call uses scratch of its own on t only:
 * planes 7 and 8 of llsm_gpu_batch_debug_plane stay what the last llsm_gpu_batch_select left, and that call does not touch
 * planes 10 and 11.
 *
 * The rules.  T, B, f, d and c are those of S1, which applies unchanged; everything is float32, one rounding per
 * operation, no contraction, every sum over k ascending.  A frame has up to 16 states: slots 0 ... 7 are near slots,
 * slots 8 ... 15 follower slots.
 *  C1. Near slots.  Slots 0 ... 7 of a frame are rule S2 unchanged: the same (c, f) in the same order; n_u as in S2.
 *  C2. First frame of an utterance.  The states are its near slots; acc_0[j] = c_0[j].  There are no followers.
 *  C3. Followers of frame i >= 1.  Take each present state a of frame i - 1, near and follower slots alike, with bank
 *      frame fa.  Its successor is s_a = fa + 1 if that frame lies in fa's bank utterance; otherwise it has none.  The pool
 *      holds the states a that have a successor and whose s_a is not the bank frame of any near slot of frame i.  The pool
 *      is ordered by (acc_{i-1}[a], a) ascending, acc_{i-1} being the value rule C5 left: a float32 comparison, ties --
 *      +infinity included -- to the smaller a.  The first min(8, |pool|) states fill slots 8, 9, ... of frame i in that
 *      order; a follower slot holds bank frame s_a and cost c(T[g], B[s_a]).  Distinct states have distinct bank frames,
 *      so a frame never holds one bank frame twice.  A follower is eligible under skip_own_utterance because its parent
 *      was.
 *  C4. Joins.  J(a, j) is rule S3 between every present state a of frame i - 1 and every present state j of frame i.  A
 *      follower reached from its own parent is a natural continuation and costs 0; so does a near slot whose frame is s_a.
 *  C5. Path.  S4 over up to 16 states: m starts at acc_{i-1}[a] + J(a, j) for the first present a and is replaced only
 *      by a strictly smaller value, over a ascending; the back pointer is that a; acc_i[j] = m + c_i[j].  No
 *      normalisation.  Absent slots are never predecessors or end states.  The path ends in the smallest state of least
 *      acc on the last frame; cost[u] is that acc.
 *  C6. utt, pos and cost are as in S5.
 * A target utterance's result depends on its own rows, the bank and the options only.
 * It follows that slots 0 ... 7 of plane 10 and the a, j < 8 block of plane 11 are planes 7 and 8 of
 * llsm_gpu_batch_select on the same inputs bit for bit; that cost[u] here is never above cost[u] there as float32 values
 * (the near states are a subset of the states with the same costs, float32 addition is monotone, so by induction every
 * near state's acc is no larger here, and a minimum over more states is no larger either); and that on a bank whose
 * utterances all have one frame nothing has a successor, slots 8 ... 15 are absent everywhere, and utt, pos and cost are
 * the bits of llsm_gpu_batch_select.
 *
 * Planes of llsm_gpu_batch_debug_plane, both always kept: plane 10, [t.total_frames][32]: c[0..15], then the bank frame
 * indices of slots 0 ... 15 as floats; absent slots hold 1e30f and -1.  Plane 11, [t.total_frames][256]: J at entry
 * 16 a + j; rows of first frames and entries of absent slots are 0.
 * Known limits: one wavefront per target utterance walks its frames in order, so few long utterances leave the device idle.
 * The followers are the eight pool states of lowest accumulated cost: a beam, not an exhaustive search over
 * continuations.  Plane 11 takes 1 KiB per target frame. */
int  llsm_gpu_batch_select_chain(llsm_gpu_batch* t, const llsm_gpu_batch* bank, const llsm_gpu_select_options* opt /* NULL: defaults */,
       int* utt, FP_TYPE* pos, FP_TYPE* cost /* may be NULL */);

/* ---- frame coder of a device-resident layer-1 batch: every frame <-> the vector [voicing, f0, Rd, order_spec mel-spectrum
 * points, order_bap band aperiodicities] of llsm_coder_encode_frames / llsm_coder_decode_frames (llsm.h), without leaving
 * the device.  The vectors are one more flat array, LLSM_GPU_CODE: upload, download, device_ptr, array_bytes and
 * transfer_many serve it like any other.  encode and decode are asynchronous on the context's stream; a refused call
 * returns -1, sets llsm_gpu_last_error() and writes and launches nothing.
 *
 * enable_coder     needs layer 1 on the batch; takes nspec, the lip radius and fnyq from it; orders are checked as
 *                  llsm_create_coder checks them (1 <= order_spec <= nspec - 1, order_bap >= 1, nspec - 1 a power of two
 *                  >= 32).  Allocates LLSM_GPU_CODE (zeroed) and builds the mel axis, which lives with the batch: the same
 *                  orders again do nothing, other orders reallocate the array.
 * coder_dimension  order_spec + order_bap + 3; 0 before enable_coder.
 * encode           reads F0, RD, PSD, VTMAGN, NVSPHSE; writes LLSM_GPU_CODE and nothing else.  A frame is voiced when
 *                  F0 > 0 and NVSPHSE > 0.
 * decode           writes, per frame, the rows that flattening the frame of llsm_coder_decode_frames(.., use_layer1, ..)
 *                  gives (llsm_chunk_to_flat, llsm_chunk_to_flat_l1); nhar = fnyq / max(20, f0) on voiced vectors:
 *                    F0, RD, PSD          always
 *                    use_layer1 = 1       voiced: VTMAGN, VSPHSE written, NVSPHSE = nhar, NHAR = 0 and HAS_HM = 0 (so that
 *                                         llsm_gpu_batch_tolayer0(b, 1) rebuilds the harmonics; AMPL and PHSE are not
 *                                         written); unvoiced: NVSPHSE = 0, NHAR = 0, HAS_HM = 1, layer-1 rows not written
 *                    use_layer1 = 0       NHAR = nhar, AMPL and PHSE the minimum-phase harmonics (zero beyond nhar),
 *                                         NVSPHSE = 0, HAS_HM = 1; VTMAGN and VSPHSE are not written
 *                    what llsm_create_frame leaves: EDC = 1e-5 on every channel, NHAR_E = maxnhar_e with EENV_AMPL and
 *                    EENV_PHSE zero, HAS_PSDRES = 0, PBPSYN = 0.  X, XRES, PSDRES, WHITE and the outputs are not written.
 *                  The lf_rd_clamp convention is honoured.  Afterwards the batch's lowest-F0 bound is unknown, as after a
 *                  partial upload.
 * A frame's vector and rows depend on that frame alone: not on its neighbours, the batch or its place in it.
 * Refused: a NULL batch, a batch without layer 1, coder not enabled, orders out of range, use_layer1 not 0 or 1, rows too
 * long for the kernels' LDS (three float rows of nspec bins, for decode also two rows of maxnhar harmonics and the
 * minimum-phase transform of maxnhar harmonics, within 160 KiB = 163840 bytes: every nspec enable_layer1 accepts fits with
 * maxnhar up to 1024).
 * Known limit: nhar is capped at the batch's maxnhar (the host decoder sizes its rows to the largest count instead), so a
 * vector whose f0 lies below fnyq / maxnhar loses its top harmonics. */
int llsm_gpu_batch_enable_coder(llsm_gpu_batch* b, int order_spec, int order_bap);
int llsm_gpu_batch_coder_dimension(llsm_gpu_batch* b);
int llsm_gpu_batch_encode(llsm_gpu_batch* b);
int llsm_gpu_batch_decode(llsm_gpu_batch* b, int use_layer1);

/* chunk <-> flat layer-1 rows (same row indexing as llsm_flat_params) */
typedef struct {
  int nspec, maxnhar;
  FP_TYPE* rd; int* has_rd; FP_TYPE* vtmagn; FP_TYPE* vsphse; int* nvsphse; int* pbpsyn; int* has_hm;
} llsm_flat_l1;
int llsm_chunk_to_flat_l1(llsm_chunk* src, llsm_flat_l1* dst, int frm_off);
int llsm_flat_l1_to_chunk(const llsm_flat_l1* src, int frm_off, llsm_chunk* dst);

/* Convenience wrappers in the reference's own object model: n_utt independent
 * llsm_analyze / llsm_synthesize calls fused into one batch. Arrays of
 * n_utt pointers; results[] receives caller-owned objects. */
int llsm_analyze_batch(llsm_aoptions* options, FP_TYPE** x, const int* nx,
  FP_TYPE fs, FP_TYPE** f0, const int* nfrm, int n_utt, llsm_chunk** results,
  FP_TYPE** x_ap);
int llsm_synthesize_batch(llsm_soptions* options, llsm_chunk** src, int n_utt,
  llsm_output** results);

/* Device fan-out of the two wrappers above: the utterance list is cut into blocks of `block_utterances` that a pool of
 * n_devices x workers_per_device workers pulls from one queue (one context / stream and page-locked staging per worker;
 * on one device the transfers of one worker overlap the kernels of the other; across devices the queue balances the
 * load).  No data-path collective (utterances are independent); results do not depend on the placement.
 * Defaults: $LLSM_GPU_DEVICES (1; "all" = every visible device), $LLSM_GPU_WORKERS (a quarter of the host threads, 2 .. 8:
 * these calls are bound by building the reference's container trees on the host), $LLSM_GPU_BLOCK (32);
 * arguments <= 0 keep the default.  use_l1 synthesis runs its blocks in order on one worker (host-ordered callbacks).
 * llsm_fanout_plan returns the number of blocks (and their first utterances); llsm_fanout_selftest runs the queue
 * with `workers` device-less workers and reports which one took each utterance (CPU test of the plumbing). */
int llsm_gpu_set_fanout(int n_devices, int workers_per_device, int block_utterances);
int llsm_fanout_plan(int n_utt, int block, int* starts, int cap);
int llsm_fanout_selftest(int n_utt, int workers, int* owner);

/* chunk <-> flat rows: frame i of `src` into row frm_off+i of host-side flat
 * arrays laid out like the batch (used by the wrappers above and by tests). */
typedef struct {
  int maxnhar, maxnhar_e, npsd, nchannel;
  FP_TYPE* f0; int* nhar; FP_TYPE* ampl; FP_TYPE* phse;
  FP_TYPE* psd; FP_TYPE* psdres; int* has_psdres; FP_TYPE* edc; int* nhar_e;
  FP_TYPE* eenv_ampl; FP_TYPE* eenv_phse;
} llsm_flat_params;
int llsm_chunk_to_flat(llsm_chunk* src, llsm_flat_params* dst, int frm_off);
/* Frame slabs.  The frames of a chunk that llsm_analyze_batch returns are carved out of ONE block per chunk
 * (the reference: about 25 heap blocks per frame), with the reference's own destructors and copy constructors attached:
 * llsm_container_attach / remove / copy, llsm_copy_*_inplace, llsm_delete_container on single frames and
 * llsm_delete_chunk behave as container.c / frame.c specify (copies are ordinary heap objects; the block goes when its
 * last object is deleted).  The one thing a host must not do is pass a member ARRAY of such a frame (hm->ampl,
 * nm->psd ...) to free / realloc itself.  The drop-in llsm_analyze returns ordinary heap frames -- the reference's
 * ownership rule -- unless $LLSM_FRAME_SLABS=1; $LLSM_FRAME_SLABS=0 switches slabs off everywhere.  Released blocks are
 * kept for the next chunk up to $LLSM_SLAB_POOL_MB if that is set; otherwise up to 64 MB, raised (never above
 * $LLSM_SLAB_POOL_MAX_MB, default 1024) to the slab volume the largest llsm_analyze_batch call so far produced -- what the
 * host itself had live a moment ago -- until llsm_slab_trim.
 *   llsm_slab_stats   live slabs, their bytes, bytes kept in the pool (any pointer may be NULL)
 *   llsm_slab_trim    hands the pooled blocks back to the allocator (those of the pooled outputs below as well)
 * Outputs.  llsm_synthesize returns the reference's four heap blocks (struct, y, y_sin, y_noise).  llsm_synthesize_batch
 * builds each llsm_output as ONE block -- struct and the three arrays -- taken from a pool of released blocks (three
 * 177 KB arrays per utterance were three fresh mappings and as many unmappings: more time than the synthesis itself);
 * llsm_delete_output recognises such an output and returns its block to the pool, which is kept up to
 * $LLSM_OUTPUT_POOL_MB if set, else up to the volume the largest batch call so far produced (32 MB ... 1 GB).  The arrays
 * of such an output must not be passed to free() one by one.  $LLSM_OUTPUT_POOL=0 / 1: never / from llsm_synthesize too. */
void llsm_slab_stats(long long* live_slabs, long long* live_bytes, long long* pooled_bytes);
void llsm_slab_trim(void);
/* n chunks at once: llsm_delete_chunk (llsm.h) on each; entries are set to NULL.  A chunk whose frames still lie untouched in
 * the slab llsm_analyze_batch built them in drops all its references in ONE decrement (nothing deleted, attached or regrown
 * since, every container and member pointer still inside the slab: values written through the structs do not count);
 * otherwise one walk of range checks per frame (objects a host attached itself go through their own destructors). */
void llsm_delete_chunks(llsm_chunk** chunks, int n);
/* Batch objects between calls (round 4).  llsm_analyze / llsm_synthesize and their *_batch forms run on persistent workers
 * (one context, stream and page-locked staging each); a worker also keeps the device batch of its last block -- buffers,
 * layout, filter-job and unit tables -- and reuses it when the next block has the same options, rates, utterance and frame
 * counts (equal-length segments: the usual shape of batch jobs), instead of building and tearing one down per block.
 * Results do not depend on it.  A differently shaped block replaces the kept batch; llsm_gpu_release_cached_batches()
 * releases the batches of idle workers (their device memory); $LLSM_GPU_BATCH_CACHE=0 switches the reuse off. */
void llsm_gpu_release_cached_batches(void);
int llsm_flat_to_chunk(const llsm_flat_params* src, int frm_off, llsm_chunk* dst);

/* Flat wire format of a layer-0 chunk (csrc/wire.cpp): ONE contiguous, position-independent
 * blob with the conf scalars and the flat rows above -- for caching analysed utterances on
 * disk, for sending them between ranks, or for uploading into a batch without building the
 * container tree.  The reference has no serialisation (container.c, frame.c keep ~25 heap
 * blocks per frame).  Little-endian, versioned ("LLSM2L0", version 2; version 1 is still read); row widths are the
 * largest harmonic counts present in the chunk.  Host-only.
 *   llsm_chunk_blob_size  bytes llsm_chunk_to_blob will write (0 on a chunk without conf)
 *   llsm_chunk_to_blob    returns the bytes written, or -1
 *   llsm_blob_view        validates an untrusted blob and points `view` INTO it (no copy);
 *                         0 on success; thop / fnyq / nfrm are optional outputs.  The blob's
 *                         address must be a multiple of 8 (rejected otherwise)
 *   llsm_blob_to_chunk    rebuilds a caller-owned chunk (llsm_delete_chunk), NULL if malformed
 *   llsm_blob_view_l1     the layer-1 rows of a blob (version 2 blobs of chunks that went through
 *                         llsm_chunk_tolayer1: RD, VTMAGN, VSPHSE, PBPSYN, which frames still hold an HM); view->nspec == 0
 *                         when there are none.  LLSM_FRAME_PBPEFF (a host callback) is never carried.
 *   llsm_gpu_batch_upload_blob  the rows of a blob straight into utterance `utt` of a batch (frame counts and row
 *                         widths must fit; enables layer 1 on the batch when the blob carries it) -- no container tree */
size_t      llsm_chunk_blob_size(llsm_chunk* src);
long long   llsm_chunk_to_blob(llsm_chunk* src, void* dst, size_t capacity);
int         llsm_blob_view(const void* blob, size_t bytes, llsm_flat_params* view, int* nfrm,
  FP_TYPE* thop, FP_TYPE* fnyq);
llsm_chunk* llsm_blob_to_chunk(const void* blob, size_t bytes);
int         llsm_blob_view_l1(const void* blob, size_t bytes, llsm_flat_l1* view);
int         llsm_gpu_batch_upload_blob(llsm_gpu_batch* b, int utt, const void* blob, size_t bytes);
/* utterances [utt0, utt0 + n) from blobs[0 .. n): rows gathered in page-locked staging, one copy per array and group */
int         llsm_gpu_batch_upload_blobs(llsm_gpu_batch* b, int utt0, int n, const void* const* blobs, const size_t* bytes);
/* The other direction: utterances of a resident batch as blobs, packed on the device (csrc/batch_blob.cpp) -- no row
 * download at the batch's full widths, no container tree.  The blob of utterance u is byte for byte what
 * llsm_chunk_to_blob writes for the chunk built from the utterance's downloaded rows the way llsm_blob_to_chunk builds one:
 * conf from llsm_aoptions_toconf(batch options, batch fnyq) with NFRM (and LLSM_CONF_NSPEC when the batch has layer 1),
 * llsm_flat_to_chunk, llsm_flat_l1_to_chunk with has_rd = 1 on every frame, HM removed where HAS_HM is 0.  So NHAR and the
 * AMPL / PHSE rows survive on voiced frames with HAS_HM only, NHAR_E and the envelope rows on voiced frames only, VTMAGN /
 * VSPHSE where NVSPHSE > 0, PSDRES where HAS_PSDRES is set, and the row widths are the largest surviving counts of the
 * utterance, not the batch's maxnhar / maxnhar_e.  An utterance's bytes depend on its own rows alone.
 *   llsm_blob_bytes                     host only: bytes of a version-2 blob of this shape (0 and a message on a negative
 *                                       dimension)
 *   llsm_gpu_batch_blob_sizes           sizes[k] = bytes of the blob of utterance utt0 + k as the batch stands now (the
 *                                       widths are found on the device)
 *   llsm_gpu_batch_download_blobs       utterance utt0 + k into dst[k]: capacity[k] bytes of any host memory, 8-byte aligned
 *   llsm_gpu_batch_download_blob_block  the same blobs back to back in ONE host block (8-byte aligned): blob k at
 *                                       offsets[k], offsets[n] = bytes used, every offset a multiple of 16, the bytes between
 *                                       blobs zero; a page-locked block (llsm_gpu_alloc_host) is written by the copy engine
 *                                       directly, any other goes through the batch's page-locked staging area
 * Synchronous: on return the blobs are in the caller's memory.  The calls read the batch and write nothing in it (rows,
 * lowest-F0 bound).  n == 0 returns 0.  Refused with -1 and a message, with no byte of any destination written: a NULL
 * batch, a range outside the batch, a NULL or misaligned destination (all before anything is launched); a capacity that is
 * too small (the message names the utterance and the bytes needed), a block that is too small, one utterance larger than
 * the 64 MiB staging area (after the width reduction, before anything is packed). */
size_t      llsm_blob_bytes(int nfrm, int maxnhar, int maxnhar_e, int npsd, int nchannel, int nchanfreq, int nspec);
int         llsm_gpu_batch_blob_sizes(llsm_gpu_batch* b, int utt0, int n, size_t* sizes);
int         llsm_gpu_batch_download_blobs(llsm_gpu_batch* b, int utt0, int n, void* const* dst, const size_t* capacity);
int         llsm_gpu_batch_download_blob_block(llsm_gpu_batch* b, int utt0, int n, void* block, size_t capacity, size_t* offsets);

/* ---- llsmrt stream groups (BASELINE.json config 4: many concurrent streams per GPU) ----
 * The reference's llsmrt buffer is one stream (llsmrt.h:33-54).  A group advances n_streams
 * independent streams (own noise templates, own rings, own output) by one hop per
 * llsm_rtsynth_group_feed with ONE kernel sequence; llsm_create_rtsynth_buffer is a group of
 * one.  Seeds: stream s draws from default seed + s.  fetch is a bulk, non-blocking pull of
 * up to max_samples samples of one stream (dst_p / dst_ap may be NULL) and returns the count. */
typedef void llsm_rtsynth_group;
llsm_rtsynth_group* llsm_create_rtsynth_group(llsm_soptions* options, llsm_container* conf,
  int capacity_samples, int n_streams);
void llsm_delete_rtsynth_group(llsm_rtsynth_group* g);
int  llsm_rtsynth_group_getlatency(llsm_rtsynth_group* g);
int  llsm_rtsynth_group_numoutput(llsm_rtsynth_group* g, int stream);
void llsm_rtsynth_group_feed(llsm_rtsynth_group* g, llsm_container** frames);
/* n_hops hops in one call (frames[k * n_streams + s]: stream s, hop k): a producer that is ahead of its consumer -- the
 * reference's feed only blocks on a FULL ring, llsmrt.c:489-493 -- packs and enqueues hop k + 1 while hop k is on the
 * device; on return the samples of every hop are in the rings, bit-identical to n_hops single feeds.
 * Like n_hops calls of feed it BLOCKS while a ring is full: a caller that is also the only consumer must keep
 * n_hops x (hop + 1) samples within the free room of the rings (capacity_samples - numoutput), or pull from another thread --
 * exactly the reference's rule for a producer that runs ahead (llsmrt.c:489-493). */
void llsm_rtsynth_group_feed_many(llsm_rtsynth_group* g, llsm_container** frames, int n_hops);
/* One hop of a buffer / group as ONE device submission: the copy-in, the launches and the copy-out of a feed are
 * stream-captured and replayed through an executable hipGraph that is updated in place every hop.  on = 1 / 0 switches
 * it for the process (default: $LLSM_RT_GRAPH, else off -- see DESIGN.md section 8 for the measurement), on < 0 only
 * queries; returns the previous setting.  llsm_gpu_rt_graph_hops: hops submitted that way so far. */
int       llsm_gpu_rt_graph(int on);
/* Shared-F0 tiles: frames of one utterance that carry a bit-identical F0 (fixed-F0 material, flat stretches of an F0
 * track) are analysed 16 at a time as the rows of one matrix product whose twiddles and window are formed once per
 * tile (k_harm_speech_tile).  Which frames qualify depends only on the utterance's own F0
 * row, never on the rest of the batch.  on = 1 / 0 switches the tile kernels for the process (default:
 * $LLSM_GPU_F0_TILES, else on), on < 0 only queries; returns the previous setting.  With 0 every frame takes the
 * per-frame kernels (results agree to float32 rounding; tests/test_gpu_tiles.py). */
int       llsm_gpu_shared_f0_tiles(int on);
/* Shared phasor tables of the harmonic resynthesis (k_synth_ola4): the frames one workgroup walks that carry the
 * F0 bits of the group's first voiced frame read the row / column phasors of every k-step from one LDS table instead
 * of rotating and re-seeding them per frame.  The table holds exactly the values the per-frame recurrences produce,
 * so x_res, y_sin and y are bit-identical on and off (tests/test_gpu_synth_tables.py).  on = 1 / 0 switches it for
 * the process (default: $LLSM_GPU_SYNTH_TABLES, else on), on < 0 only queries; returns the previous setting. */
int       llsm_gpu_synth_tables(int on);
/* Pulse-by-pulse synthesis (layer 1): a pulse group is real, so its inverse transform runs as ONE complex transform of
 * half its size (k_pbp_pulse, round 4: half the LDS, twice the pulse groups in flight) instead of the full-size
 * transform of the Hermitian-completed spectrum.  on = 1 / 0 switches it for the process (default on), on < 0 only
 * queries; returns the previous setting.  The samples agree to float32 rounding (tests/test_gpu_l1.py). */
int       llsm_gpu_pbp_real_ifft(int on);
/* The Kalman smoother of an analysis on a second stream beside the band filter and the envelope analysis (it needs
 * nothing they produce and is bound by HBM where they are bound by arithmetic); joined before the call returns its
 * work to the context's stream, so callers see one stream.  on = 1 / 0 for the process (default: $LLSM_GPU_OVERLAP,
 * else on), on < 0 only queries; returns the previous setting.  Results do not depend on it. */
int       llsm_gpu_analysis_overlap(int on);
long long llsm_gpu_rt_graph_hops(void);
/* Kernel launches per hop of a buffer / group.  0: five single-purpose launches.  1: two -- envelope frames beside the
 * harmonic frame, ring adds and excitation in the first; noise filter (four wavefronts per pair of streams), noise ring
 * and the hop's output samples in the second; a pulse-by-pulse buffer's dual-buffer bookkeeping rides in the first.
 * 2: one -- a workgroup of 512 threads takes a pair of streams through both (transforms of at most 2048 points).
 * 3 (default): one, with the hop's temporaries in LDS and every ring cell read and written once (k_rt_hop2; windows of at
 * most 1024 samples, transforms of at most 2048 points, else as 2).  A pulse-by-pulse hop on which pulse groups are
 * due adds the pulse kernel in front.  Sets the mode for the process (default: $LLSM_RT_FUSED, else 3), on < 0 only
 * queries; returns the previous setting.  1, 2 and 3 give bit-identical samples; 0 differs from them by the float32
 * rounding of the noise part. */
/* Pipelined feeds (round 4).  A feed is synchronous by default, as llsmrt.c's is: when it returns, the hop's samples are in
 * the rings.  With on = 1 a feed returns as soon as the hop is enqueued; its samples are appended when the NEXT feed
 * starts, when a fetch or a numoutput call finds the stream's ring empty (it then waits for the hop in flight), or on
 * clear -- so a consumer that pulls blocks while numoutput allows sees them one hop later (one hop of extra latency), a
 * consumer that drains to zero after every feed gets the reference's behaviour without the overlap, and the host side
 * of a hop (pulls, packing the next frames) runs beside the device instead of after it.  The samples are the same.  Hops that write rebuilt harmonic
 * models back onto the caller's frames stay synchronous.  Default: $LLSM_RT_PIPELINE, else off; on < 0 only queries;
 * returns the previous setting. */
int       llsm_gpu_rt_pipeline(int on);
int       llsm_gpu_rt_fused(int on);
/* The kernels of a (one- or two-launch) hop read the hop's parameter rows from the pinned host block and write
 * the hop's samples into the pinned host block themselves, instead of a copy launch before and after them (the rows
 * hold nfft harmonic slots of which a frame uses a few hundred; each copy was a dependent launch about as long as one of
 * the kernels).  Same kernels, same arithmetic: the samples are bit-identical.  on = 1 / 0 switches it for the process
 * (default: $LLSM_RT_DIRECT, else on), on < 0 only queries; returns the previous setting.  Hops of a pulse-by-pulse buffer
 * that rebuild harmonic rows on the device and hops replayed as a graph keep the copy in. */
int       llsm_gpu_rt_direct(int on);
int  llsm_rtsynth_group_fetch(llsm_rtsynth_group* g, int stream, FP_TYPE* dst_p, FP_TYPE* dst_ap,
  int max_samples);
/* every stream at once (a mixer's pull): row s of dst_p / dst_ap -- [n_streams][max_samples], either may be NULL --
 * receives up to max_samples samples of stream s; counts (n_streams ints, may be NULL) gets the samples per stream;
 * returns the smallest count. */
int  llsm_rtsynth_group_fetch_all(llsm_rtsynth_group* g, FP_TYPE* dst_p, FP_TYPE* dst_ap, int max_samples,
  int* counts);

/* Seed used by llsm_synthesize / llsm_create_rtsynth_buffer (the reference
 * draws from libc rand(), dsputils.c:357; here every call advances a
 * process-wide counter starting from this seed). */
void llsm_gpu_set_default_seed(unsigned long long seed);

/* Index plan exported for tests: same float32
 * evaluation the kernels use. which: 0 center(i) 1 nwin_sin 2 nwin_env
 * 3 nwin_filt 4 nwin_psd 5 ny(i=nfrm) 6 hwin(f0) 7 nhar(f0,i=maxnhar)
 * 8 env_ola(i,j) 9 dcwin(f0) 10 spgmwin(f0,i=nwin_psd) 13 time segments
 * the zero-phase band filter cuts a signal of i samples into when its slowest
 * pole reaches j samples (1: whole).  A function of the signal alone, so an
 * utterance gets the same bits in every batch.  14 frames per unit of the
 * harmonic overlap-add for a one-utterance batch of i frames, maxnhar j.
 * 15 first output sample of unit j of the noise excitation in an utterance of
 * i samples, -1 past its last unit.  16 how the zero-phase band filter treats
 * a signal of i samples in the band [f0, thop] Hz (the two arguments carry
 * fmin and fmax) at fs; j selects: 0 M, the samples each end job of a fused
 * band-pass writes, and 1 M' = 2 M + 64, the stretch it filters (0: the band
 * is a single low- or high-pass); 2 whether i samples run fused (i >= 4 M');
 * 3 the halo of a time segment; 4 the number of time segments; 5 and 6 the
 * range [lo, hi) the main job or its segments write ([M, i - M) when fused);
 * 100 + s the first sample segment s writes.
 * 17 the kernel that filters the noise of an offline synthesis at hop thop
 * and rate fs with PSD rows of j points, under the Hann convention in force:
 * i != 0 the fused filter + overlap-add is wanted (the default), i == 0 it is
 * not ($LLSM_GPU_NOISE_OLA=0).  100 + 10 ALIAS + TQ: k_noise_filter_ola<LOGN,
 * ALIAS, TQ>; 1 k_noise_filter_wf<LOGN>; 2 k_noise_filter on the LDS; 3 on
 * global scratch (the last three followed by k_ola_noise_mix).
 * 18 frames per unit of the fused noise filter for an utterance of j frames
 * in a batch of i frames, under $LLSM_GPU_NOISE_UNIT as it stands.
 * -1: no such quantity. */
int llsm_gpu_plan_index(int which, int i, int j, FP_TYPE f0, FP_TYPE thop,
  FP_TYPE fs, FP_TYPE rel_winsize);

#ifdef __cplusplus
}
#endif
#endif
