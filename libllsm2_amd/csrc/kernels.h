// kernels.h -- host-side view of the HIP kernels (kernels.hip): plain structs
// and one launch function per kernel.  engine.cpp sequences them.
#ifndef LLSM_AMD_KERNELS_H
#define LLSM_AMD_KERNELS_H

// Build switches of experiments only.  Timing ablations and deliberately wrong builds (KAL_ABL, NF_ABL, KAL_BREAK and the
// hooks of tools/kbench_experiments.h) and the tuning constants below (their defaults sit beside their kernels) can only be
// set together with -DLLSM_KBENCH_EXPERIMENTS, which tools/kbench.py --build adds: a stray -D of one of them is a compile
// error instead of a product library that is slow, spills or computes garbage.  Every kernel source and engine.cpp include
// this header before any other of the library's, so the names are tested before a header sets a default.
#if ! defined(LLSM_KBENCH_EXPERIMENTS) && ( \
    defined(KAL_ABL) || defined(NF_ABL) || defined(KAL_BREAK) || defined(IIR_FAKE_L2) || defined(IIR_GEN_EXPERIMENT) || \
    defined(RT2_TIMING) || defined(HT_TABLE_EXPERIMENT) || \
    defined(HT_SEG) || defined(HT_CHUNK) || defined(HT_WPE) || defined(HE_WPE) || defined(IIR_SEG) || defined(IIR_WPE) || \
    defined(KAL_WPE) || defined(KAL_CHUNK) || defined(EXU_Q) || defined(EXU_WPE) || defined(NF_OLA_WPE) || \
    defined(SO4_WAVES) || defined(SO4_WPE) || defined(PBP_NT) || defined(PBP_WIDE_BELOW) || defined(PBP_WPE) || \
    defined(SYN_UNIT_DIV) || defined(NF_UNIT_DIV))
#error "experiment build switches need -DLLSM_KBENCH_EXPERIMENTS (tools/kbench.py --build); the product library is never built with them"
#endif

#include <hip/hip_runtime.h>
#include <stddef.h>
#include "cheby.h"                                // IIR_SEG
#include "packed.h"                               // LlsmPackedLayout

// One 4th-order Chebyshev-I section in transposed direct form II (cheby.h)
// with everything the wave-parallel block recursion needs, all float64:
// steady-state initial conditions zi, the state-transition powers
// M[d] = (A^IIR_SEG)^(2^d) (row-major 4x4) and the zero-input output rows
// H[i] = e0^T A^i.
struct FiltSectionD {
  double b[5];
  double a[5];
  double zi[4];
  double M[6][16];
  double H[IIR_SEG][4];
};

// One zero-phase filtering job: src -> [sec0] -> (mid -> [sec1]) -> dst.
#ifndef KAL_CHUNK
#define KAL_CHUNK 8                                  // frames per chunk of k_kalman: checkpoint spacing (engine.cpp sizes the checkpoint rows with it) and rows per request
#endif
struct FiltJob {
  const float* src;
  float* dst;
  float* mid;    // only used when sec1 >= 0
  float* tmp;    // n + 30 floats (forward-pass output)
  int n;
  int sec0;
  int sec1;      // -1: single section
  int square;    // dst = y*y (llsm_subband_energy)
  int pad;       // odd-extension length of filtfilt (0: the default 15)
  int fused;     // two sections per pass (k_filtfilt): only the interior [wlo, whi) is valid
  int wlo, whi;  // samples of dst this job writes; whi <= wlo: all n
};

// switchable conventions of the ciglet primitives the reference cannot confirm
struct DevConventions {
  int mavg_half;       // moving_avg(x, n, 3): half width 3 (7 taps, default) or 1 (3 taps)
  int interp1u_excl;   // interp1u's right end: 0 inclusive (default), 1 exclusive
  int kalman_init;     // kalmanf1d at the first frame: 0 x0 = z0, P0 = R0 (default); 1 x0 = z0, P0 = the filter update of the prior P = R0
  float lobe_bias;     // cig_spec2env: constant added to the log envelope (layer 1); default 0.13397922601295542
  int lf_rd_clamp;     // lfmodel_from_rd: 0 extension formulas outside 0.21 <= Rd <= 2.7 (default); 1 Rd limited to 0.3 .. 2.7
};
int llsm_l1_kernels_set_conventions(const DevConventions& c);
int llsm_kernels_set_conventions(const DevConventions& c);

// Device-resident description of a batch (all pointers are device pointers).
struct BatchDev {
  int n_utt, nframes;
  int maxnhar, maxnhar_e, npsd, nchannel;
  float thop, fs, rel_winsize;
  // per utterance
  const int* x_off; const int* nx; const int* frm_off; const int* nfrm;
  // per frame
  const int* frm_utt;
  float* f0; int* nhar; float* ampl; float* phse;
  float* psd; float* psdres; int* has_psdres; float* edc; int* nhar_e;
  float* eenv_ampl; float* eenv_phse;
  // waveforms
  const float* x;
  // frame pairs sharing one complex transform in the PSD / envelope kernels: (g0, g1 or -1),
  // both of one utterance, so that a frame's result does not depend on its batch neighbours.
  // NULL = global pairing (2p, 2p + 1).
  const int2* pairs; int npairs;
  // 16-aligned blocks of every utterance's frames: (first global frame, frames in the block); the units of
  // k_harm_speech_tile.  NULL: no tiles.
  const int2* hblocks; int nhblocks;
  // k_synth_ola4: phasor tables shared by the frames of one F0 (0: every frame runs its own recurrences; same bits)
  int synth_tables;
};

// Transforms beyond the LDS kernels (N > LLSM_LDS_FFT_MAX points: a 25 ms hop at 96 kHz, peak picking below 21.6 Hz): the
// in-place FFT of dev_common.h run on per-workgroup GLOBAL scratch with twiddles from a table of its own
// (e^{-2 pi i m / tw_big_nmax}); engine.cpp llsm_engine_big_fft provides both before such a launch.
#define LLSM_LDS_FFT_MAX 8192
#define LLSM_BIG_FFT_MAX (1 << 17)
#define LLSM_BIG_FFT_GRID 512                          // persistent workgroups of a big-transform launch, at most
// ... fewer when a workgroup's scratch slice is large: the scratch of a launch stays within 256 MB (a 2^17-point peak-picking
// launch -- a batch whose lowest F0 is unknown provisions for it -- gets 170 workgroups instead of 512 x 1.5 MB)
static inline int llsm_big_fft_grid(size_t elems_per_wg) {
  const size_t cap = ((size_t)256 << 20) / sizeof(float2) / (elems_per_wg ? elems_per_wg : 1);
  return (int)(cap < 16 ? 16 : (cap > LLSM_BIG_FFT_GRID ? LLSM_BIG_FFT_GRID : cap));
}

struct LaunchCtx {
  hipStream_t stream;
  void (*prof_begin)(void* user, const char* name, hipStream_t stream);   // (events go on the stream of the launch)
  void (*prof_end)(void* user, hipStream_t stream);
  void* prof_user;
  const float2* tw_big = nullptr; int tw_big_nmax = 0; float2* big_scratch = nullptr; size_t big_scratch_elems = 0;
};

int launch_refine_f0(LaunchCtx* P, const BatchDev& d);
int launch_harm_speech(LaunchCtx* P, const BatchDev& d, float min_f0);
int launch_harm_env(LaunchCtx* P, const BatchDev& d, const float* ce, size_t ce_stride);
int launch_synth_frames(LaunchCtx* P, const BatchDev& d, int nwin, const float* win,
  const float* cyc_shift, float* frames, int lds_harmonics);
int synth_ola_group_units(void);
int synth_ola_unit_div(int nwin, int lds_harmonics);
int launch_synth_ola(LaunchCtx* P, const BatchDev& d, const int4* units, int nunits, int halo,
  int nwin, const float* win, int lds_harmonics, const int* out_off, const int* out_len,
  const float* x, float* out, int mode, float* mix);
int launch_harm_pp_big(LaunchCtx* P, const BatchDev& d, const float* sig, size_t sig_stride, int nsig,
  const int* nfft_u, int maxnhar, float norm_base, int lds_n, int nmax, int* nhar_out, float* ampl, float* phse);
int launch_filtfilt(LaunchCtx* P, const FiltJob* jobs, int njobs, const FiltSectionD* sections);
int launch_wf_selftest(LaunchCtx* P, int logN, const float2* in, float2* out, int count, int inverse);
int launch_spgm_env(LaunchCtx* P, const BatchDev& d, int nwin_psd, int N, int logN,
  int nfft_psd, float norm_base, const float2* tw, int tw_nmax, float* env_out,
  int2* fix_list, int* fix_count, int which = 3);   // fix_list [number of frame pairs] / fix_count: pairs whose DC / Nyquist bin the second launch recomputes exactly (NULL: off)
int launch_psd_frames(LaunchCtx* P, const BatchDev& d, const float* xres, int nwin,
  const float* win, float inv_wpow, int N, int logN, const float2* tw, int tw_nmax,
  float* psd_log);
int launch_kalman(LaunchCtx* P, const BatchDev& d, const float* env, const float* psd_log,
  float* ck, int nspec);
int launch_white(LaunchCtx* P, const BatchDev& d, float* white, int ntemplate_ext,
  const int* out_len, unsigned long long seed);
int launch_env_frames(LaunchCtx* P, const BatchDev& d, float fs_syn, int nwin,
  const float* win, float* envf);
#define LLSM_EXC_HITS 3                              // envelope frames that can cover one output sample
int launch_env_params(LaunchCtx* P, const BatchDev& d, float2* cplx);
int launch_pack_frames(LaunchCtx* P, const BatchDev& d, const LlsmPackedLayout& L, float* out, float* const* dst_tab);
int launch_unpack_frames(LaunchCtx* P, const BatchDev& d, const LlsmPackedLayout& L, const float* in, const float* const* src_tab);
int launch_scatter_outputs(LaunchCtx* P, int n_utt, int max_ny, const float* y, const float* ysin, const float* ynoise,
  const int* y_off, const int* ny, float* const* tab);
int launch_env_plan(LaunchCtx* P, int max_ny, int max_nfrm, int nwin_env, float thop, float fs, int2* hits, int* over);
// cplx == NULL: k_excite_units over `units` (two int4 per unit: {u, s0, samples, ny}, {frm_off, nfrm, y_off, 0}), which
// forms the complex amplitudes itself; otherwise the k_env_params rows feed k_excite_env
int launch_excite_env(LaunchCtx* P, const BatchDev& d, const float* colored, int ntemplate_ext,
  const int2* hits, const float2* cplx, int nwin_env, const float* win, int nch_active,
  const int* out_off, const int* out_len, int max_len, float fs_syn, float* yexc,
  const int4* units = nullptr, int nunits = 0);
bool excite_units_ok(const BatchDev& d, int nwin_env, float fs_syn);   // the geometry k_excite_units takes
int excite_unit_samples();                            // output samples per unit of k_excite_units
// Which kernel filters the noise of a 2^logN-point transform with target rows of npsd points (llsm_gpu_plan_index case 17;
// both launchers below decide by it, so the value is the kernel that runs).  fused: the caller wants filter and overlap-add
// in one kernel.  Fused: 100 + 10 ALIAS + TQ of k_noise_filter_ola<LOGN, ALIAS, TQ>; otherwise -- fused not wanted, or no
// fused instantiation at this size -- k_noise_filter_wf<LOGN>, or k_noise_filter on the LDS or on global scratch.
enum { NF_ROUTE_WF = 1, NF_ROUTE_LDS = 2, NF_ROUTE_SCRATCH = 3, NF_ROUTE_FUSED = 100 };
int noise_filter_route(int logN, int npsd, int wsym, bool fused);
int launch_noise_filter(LaunchCtx* P, const BatchDev& d, const float* yexc,
  const int* out_off, const int* out_len, float fnyq_conf, float fs_syn, int nwin,
  const float* win, float inv_wsqr, int N, int logN, const float2* tw, int tw_nmax,
  float* nframes_out, int* live, int rt);
int launch_noise_filter_ola(LaunchCtx* P, const BatchDev& d, const int4* units, int nunits, int halo,
  const float* yexc, const int* out_off, const int* out_len, float fnyq_conf, float fs_syn, int nwin,
  const float* win, int wsym, float inv_wsqr, int logN, float* ynoise);   // wsym: win[j] == win[wsym - j] (0: no such symmetry)
int launch_ola_noise_mix(LaunchCtx* P, const BatchDev& d, const float* nframes_in,
  const int* live, int N, const int* out_off, const int* out_len,
  int max_len, float fs_syn, const float* ysin, float* ynoise, float* y);

int launch_utt_fftsize(LaunchCtx* P, const BatchDev& d, int nmax, int* nfft_u);
int launch_harm_pp(LaunchCtx* P, const BatchDev& d, const float* sig, size_t sig_stride, int nsig,
  const int* nfft_u, int maxnhar, float norm_base, const float2* tw, int tw_nmax, int lds_n,
  int* nhar_out, float* ampl, float* phse);
int launch_rt_template(LaunchCtx* P, const float* colored, int ntemplate_ext, int nch, int nch_active,
  int ntemplate, int S, float* tpl);

// ---- llsmrt: one hop of one stream group (rt.cpp)
// the per-stream parameter rows of a hop where the host packed them (pinned, device-mapped); f0 == nullptr: none
struct RtPbpOp;
struct RtRows {
  const float *f0, *cyc, *ampl, *phse, *edc, *eamp, *ephs, *psd;
  const int *nhar, *nhar_e, *has_nm;
  const float* f0sin; const RtPbpOp* ops;           // pulse-by-pulse buffers (else nullptr): -> the device f0_sin / ops rows
};
// pulse-by-pulse bookkeeping of the hop inside k_rt_front / k_rt_hop (k_rt_pbp's arguments); ops == nullptr: none
struct RtPbpArgs { RtPbpOp* ops; float* frwd; float* bkwd; int dual_curr; const float* pulse_out; int pulse_stride; };
// Everything the device work of one hop reads.  rt.cpp fills one per hop (rt_hop_record); a launcher below unpacks it, and
// is the only place that knows the parameter order of its kernel.
struct RtHop {
  // stream rows: the S streams as a batch of S one-frame "utterances" (d.f0: F0 of the envelope frames; f0_sin: of the
  // harmonic frames -- the same row unless the buffer synthesises pulse by pulse)
  BatchDev d; const float* f0_sin; const float* cyc_shift; const int* has_nm;
  // window (Hann, nwin = 2 nhop) and the transform of the noise filter
  int nwin; const float* win; float inv_wsqr; int N, logN; const float2* tw; int tw_nmax; float fnyq; int lds_harmonics;
  // rings [S][cap] (mod: [S][nchannel][cap]) and their cursors as the kernels of THIS hop must see them (the dual buffer's:
  // pbp.dual_curr); excitation templates [S][nchannel][ntemplate]
  float *mod, *sinr, *noiser, *excr; int cap;
  int mod_curr, sin_curr, noise_curr, exc_curr, exc_cycle, sin_pos;
  const float* tpl; int ntemplate;
  // temporaries of the hop (k_rt_hop2 keeps them on chip); hop lengths and the output rows [S][2][out_stride]
  float *envf, *frames_sin, *exc_frame, *nframes; int* live;
  int nhop, next_nhop, out_stride; float* out;
  // host.f0 != nullptr: every workgroup first moves its stream's rows (as many harmonics as the frame has) from the pinned
  // rows into the device rows of d / cyc_shift / has_nm, then works on those
  RtRows host; RtPbpArgs pbp;
};
// The form a hop takes under llsm_gpu_rt_fused(mode): five single-purpose launches (mode 0); k_rt_front + k_rt_back (1, and
// 2 / 3 where the LDS of one launch does not hold the transform); k_rt_hop (2); k_rt_hop2, the hop's temporaries on chip
// (3, where its per-thread slots and its LDS hold the hop; else k_rt_hop)
enum RtHopForm { RT_HOP_FIVE, RT_HOP_TWO, RT_HOP_ONE, RT_HOP_CHIP };
RtHopForm rt_hop_form(const RtHop& h, int mode);
int launch_rt_front(LaunchCtx* P, const RtHop& h);    // envelope frames beside the harmonic frame, ring adds, excitation
int launch_rt_back(LaunchCtx* P, const RtHop& h);     // noise filter of a pair of streams, noise-ring add, output samples
int launch_rt_hop(LaunchCtx* P, const RtHop& h);      // RT_HOP_ONE: both halves in one launch
int launch_rt_hop2(LaunchCtx* P, const RtHop& h);     // RT_HOP_CHIP
// the single-purpose kernels.  launch_rt_rings and launch_rt_excite also run outside a hop (rt.cpp blank_heads,
// reset_state) on a record of which they read the rings, cursors and rows only; the excitation mixer's span is explicit
int launch_rt_rings(LaunchCtx* P, const RtHop& h);
int launch_rt_rings_excite(LaunchCtx* P, const RtHop& h);
int launch_rt_excite(LaunchCtx* P, const RtHop& h, int curr_nhop, int nx, int nwin_frame);
int launch_rt_mix(LaunchCtx* P, const RtHop& h);


// ---- layer 1 / pulse-by-pulse synthesis (l1_kernels.hip) ----
struct AlphaCache { double* alpha; float* rd; float* f0; };   // alpha: 9 float64 per frame, the whole lf::Solved (l1_kernels.hip lf_solve_cached)
struct L1Dev {
  int nframes, maxnhar, nspec;
  float fnyq, lip_radius;
  const float* f0; int* nhar; float* ampl; float* phse;
  float* rd; float* vtmagn; float* vsphse; int* nvsphse; int* has_hm;
  // tolayer1 only (may be NULL / 0): scratch rows [nframes][maxnhar] for the source-removed amplitudes, and the
  // per-utterance frame pairs (BatchDev::pairs) of the two-frames-per-transform envelope kernel
  float* src_ampl; const int2* pairs; int npairs;
  // alpha of the frame's LF model (the wavefront search of lf_solve_wave), kept per frame with the (Rd, F0) it was solved
  // for: the four kernels of a layer-1 step that need it solve it once (acache.alpha NULL: no cache)
  AlphaCache acache;
};
// one pulse group = the pulses of one frame (llsm_make_filtered_pulse's arguments, llsmutils.c:132-134)
struct PbpJob {
  int frame;        // global frame index (rows of f0 / rd / vtmagn / vsphse)
  int first, npulse;// pulses[first .. first + npulse)
  int size;         // pulse_size (power of two)
  int pre_rotate;
  int out_off;      // offset of this group's `size` samples in the pulse buffer
  int start;        // output sample of pulse sample 0 (within the utterance / ring)
  int zero_extra;   // pulse sample that ALSO lands on output sample 0 through (int) truncation, or -1
};
struct PbpPulse { double T0, te, tp, ta, Ee; float offset; float pad; };
// one stretch of the HM <-> PbP cross-fade curve (layer0.c:240-262)
struct PbpSeg { double state, rate; int j0, j1, dir, len; int out_off, pad; };

// llsmrt, PbP path: per-stream operations of one hop on the dual (pulse) buffer and the sinusoid ring
struct RtPbpOp { int add_off, add_size, rd_off, rd_on, term_off, term_size, pad0, pad1; };
int launch_rt_pbp(LaunchCtx* P, const RtHop& h);       // k_rt_pbp on h.pbp (the five-launch form; the others carry it)
int launch_coder_encode(LaunchCtx* P, int order_spec, int order_bap, int ns, int npsd, float fnyq, float liprad,
  const float* melaxis, int nframes, const float* f0, const float* rd, const float* psd, const float* vtmagn,
  const int* nvsphse, float* enc);
int launch_coder_decode(LaunchCtx* P, int order_spec, int order_bap, int ns, int npsd, int maxnhar, float fnyq, float liprad,
  const float* melaxis, float mel_floor, float mel_ceil, int nframes, const float* enc, int use_l1, const float2* tw,
  int tw_nmax, float* f0, float* rd, int* nhar, float* ampl, float* phse, float* psd, float* vtmagn, float* vsphse,
  int* nvsphse, int* has_hm);
int l1_minphase_nmax(int maxnhar);
int launch_l1_rd_fit(LaunchCtx* P, const L1Dev& d, const float* model_power, const float* model_param,
  const double* inv_t, const double* cumlog_t, float* rd_raw);   // inv_t / cumlog_t: [nh (+ 1)][64] float64 tables, NULL: per-term form
int launch_l1_rd_smooth(LaunchCtx* P, int n_utt, const int* frm_off, const int* nfrm, int order,
  const float* rd_raw, int* prev_idx, int* next_idx, float* cont, float* rd_out);
int launch_l1_frame(LaunchCtx* P, const L1Dev& d, int nfft, const float2* tw, int tw_nmax);
int launch_l1_to_l0(LaunchCtx* P, const L1Dev& d, int maxnhar_conf, int only_missing, const int* select,
  const float2* tw, int tw_nmax);
int launch_pbp_pulse(LaunchCtx* P, const L1Dev& d, const PbpJob* jobs, int njobs, const PbpPulse* pulses,
  int size_max, float fs, const float2* tw, int tw_nmax, float* out);
// next-cycle projection of every layer-1 frame (layer0.c:181-191), float64
int launch_l1_projection(LaunchCtx* P, const L1Dev& d, double fs, double* proj);
int launch_l1_mixcurve(LaunchCtx* P, const PbpSeg* segs, int nsegs, float* mixw);
int launch_pbp_mix(LaunchCtx* P, int n_utt, int max_len, const int* out_off, const int* out_len, const int* frm_off,
  const int* nfrm, float thop, float fs, int nwin, const float* hm_frames, const float* f0_hm, const PbpJob* jobs,
  const int2* blk_jobs, const int* blk_off, const float* pulse_buf, const float* mixw, const float* ynoise,
  float* ysin, float* y);

// ---- edits of a device-resident batch (modify_kernels.hip, modify.cpp) ----
// Every parameter row of one batch; the layer-1 pointers are NULL (and nspec 0) when the batch has no layer 1.
struct ModRows {
  int nframes, maxnhar, maxnhar_e, npsd, nchannel, nspec;
  float* f0; int* nhar; float* ampl; float* phse; float* psd; float* psdres; int* has_psdres; float* edc; int* nhar_e;
  float* eenv_ampl; float* eenv_phse;
  float* rd; float* vtmagn; float* vsphse; int* nvsphse; int* pbpsyn; int* has_hm;
};
// theta == NULL: each frame is shifted by minus its reference phase (llsm_frame_phasesync_rps); else by theta[frame]
int launch_phase_shift(LaunchCtx* P, const ModRows& r, const float* theta, int layer1_based);
// theta[frame] = (float)(running float32 sum of the utterance's F0 up to the frame x k2pi), llsm_chunk_phasepropagate
int launch_phase_propagate_theta(LaunchCtx* P, int n_utt, const int* frm_off, const int* nfrm, const float* f0,
  double k2pi, float* theta);
// Map of llsm_gpu_batch_retime and llsm_gpu_batch_splice with the utterances resolved on the host: side A of output frame g
// is the pair rule (modify_kernels.hip) on src's frames ga[g] and ga[g] + 1 (flat frame indices) at weight ra[g] -- the second
// is read only where ra[g] != 0 --, side B the same of gb / rb, and the output the pair rule on (A, B) at weight mix[g].  gb,
// rb and mix NULL: side A alone.  gr[g]: the flat source frame of the PSDRES row, NULL: the frame at floor(pos) of side A below
// mix 0.5, of side B from there on.
struct SpliceMap { const int* ga; const float* ra; const int* gb; const float* rb; const float* mix; const int* gr; };
int launch_splice(LaunchCtx* P, const ModRows& src, const ModRows& dst, const SpliceMap& m);
// llsm_gpu_batch_pitch_formant over frames [g_lo, g_hi) (every edited frame): rho / alpha are per-frame F0 and formant
// ratios (NULL: 1), warp_psd the PSD warp; LDS: 16 (nspec + npsd) bytes per workgroup
int launch_pitch_formant(LaunchCtx* P, const ModRows& r, int g_lo, int g_hi, const float* rho, const float* alpha,
  int warp_psd);
// llsm_gpu_batch_smooth.  A tile is up to kSmoothTile frames g0 ... g0 + cnt - 1 of one utterance (flat frames u0 ... u1),
// every one with a radius > 0; its frames are entries slot ... slot + cnt - 1 of the compact list: `radius` holds their
// radii, `rows` one result row [VTMAGN | PSD | EDC | F0, RD] (smooth_row_width floats) each, and `mark` what the store does
// with each (0: S3, left alone; 1: unvoiced; 2: voiced).  launch_smooth_rows reads the batch and writes rows and mark only;
// launch_smooth_store, behind it on the same stream, writes the batch.  flags: LLSM_GPU_SMOOTH_*.
const int kSmoothTile = 16, kSmoothMaxRadius = 32;
enum { SM_F0 = 1, SM_RD = 2, SM_VTMAGN = 4, SM_PSD = 8, SM_EDC = 16 };   // LLSM_GPU_SMOOTH_* (modify.cpp asserts it)
struct SmoothTile { int g0, cnt, u0, u1, slot; };
struct SmoothJob { const SmoothTile* tiles; int ntiles; const int* radius; float* rows; int* mark; int flags; };
inline int smooth_row_width(const ModRows& r) { return r.nspec + r.npsd + r.nchannel + 2; }
int launch_smooth_rows(LaunchCtx* P, const ModRows& r, const SmoothJob& job);
int launch_smooth_store(LaunchCtx* P, const ModRows& r, const SmoothJob& job);

// ---- frame coder of a device-resident batch (batch_coder.cpp): launch_coder_encode / launch_coder_decode above on the batch's
// rows, then the members the host decoder leaves at their llsm_create_frame values (coder_kernels.hip)
int launch_batch_decode_rest(LaunchCtx* P, const ModRows& r, int use_l1);

// ---- export of a device-resident batch as chunk blobs (batch_blob.cpp, blob_kernels.hip; byte layout: wire_layout.h)
namespace llsm_wire { struct BlobEntry; }
// widths[3 k + 0 / 1 / 2]: the largest NHAR, NVSPHSE and NHAR_E that survive in the blob of the utterance whose frames are
// frm_off[k] .. frm_off[k] + nfrm[k] (k < n)
int launch_blob_widths(LaunchCtx* P, const ModRows& r, const int* frm_off, const int* nfrm, int n, int* widths);
// every byte of the n blobs of `tab` into `stage` (16-byte aligned): header, chanfreq (nchanfreq floats), rows at the
// blob's own widths, zero padding, and the gap up to the next multiple of 16 behind each blob
int launch_blob_pack(LaunchCtx* P, const ModRows& r, const llsm_wire::BlobEntry* tab, const float* chanfreq, int n,
  int max_nfrm, unsigned char* stage);

// ---- F0 estimation of a batch's waveforms (f0.cpp, f0_kernels.hip; rules: llsm_gpu.h)
// The batch's tables and waveforms, the sizes of llsm_gpu_f0_plan and the two float options as the float64 values the
// rules compare against: threshold, and gate = silence_rel^2
struct F0Dev {
  int n_utt, nframes; float thop, fs;
  const int* x_off; const int* nx; const int* frm_off; const int* nfrm; const int* frm_utt;
  const int2* pairs; int npairs;                       // BatchDev::pairs: the two frames of one transform
  const float* x;
  int lmin, lmax, W;
  double threshold, gate;
};
int launch_f0_energy(LaunchCtx* P, const F0Dev& d, double* uss);            // uss[u] = sum of x^2 over utterance u, float64
// What the candidate search of llsm_gpu_batch_track_f0 adds (rule T1): the plane [nframes][24], cand_threshold, and
// L = (float)log2(fs / lmin).  plane == NULL: the lag search of estimate_f0 (rules 6 - 7) into raw.
struct F0Cand { float* plane; float threshold, L; };
// the four costs of rules T2 - T3
struct F0Track { float unvoiced, sw, jump, octave; };
// raw[g]: rules 2 - 7 of frame g, or with c.plane the candidate row of frame g and raw not written; cmndf (or NULL):
// [nframes][lmax + 1]; logN: log2 of the transform, 8 ... 12
int launch_f0_cmndf(LaunchCtx* P, const F0Dev& d, int logN, const double* uss, float* raw, float* cmndf, const F0Cand& c);
int launch_f0_median(LaunchCtx* P, const F0Dev& d, const float* raw, float* f0);   // rule 8
// rules T2 - T5 over the candidate plane: f0[nframes]; bp: one word per frame of scratch
int launch_f0_viterbi(LaunchCtx* P, const F0Dev& d, const float* plane, const F0Track& t, unsigned* bp, float* f0);

// ---- alignment of utterance pairs: whole matrix, inside a diagonal band, whole matrix under the slope pattern, the slope
// pattern inside the band, or either pattern inside a band around a centre line of the caller's (align.cpp,
// align_kernels.hip; rules D1 - D3, B1 - B4, L1 - L4, K1 - K4 and A1 - A3: llsm_gpu.h)
// The centre column of row i of an na x nb pair, rule B1: the diagonal rounded half up.  Row i spans columns
// max(0, c - band) ... min(nb - 1, c + band); entry q of its row of the band plane is column c - band + q.
__host__ __device__ static inline int align_band_center(int i, int na, int nb) {
  return na > 1 ? (int)((2ll * i * (nb - 1) + (na - 1)) / (2ll * (na - 1))) : 0;
}
// The columns lo ... hi of row i of an admissible na x nb pair under the slope pattern, rule L1 (llsm_gpu_batch_align_slope):
// the cells from which (0, 0) is reached backwards and (na - 1, nb - 1) forwards.  lo > hi: no path stops on the row.
__host__ __device__ static inline void align_slope_row(long long i, int na, int nb, int& lo, int& hi) {
  const long long r = (long long)na - 1 - i, l0 = (i + 1) / 2, l1 = (long long)nb - 1 - 2 * r, h0 = 2 * i,
                  h1 = (long long)nb - 1 - (r + 1) / 2;
  lo = (int)(l0 > l1 ? l0 : l1); hi = (int)(h0 < h1 ? h0 : h1);
}
// The columns lo ... hi of row i of a query against a take of nb frames under the slope pattern with free ends, rule Q1
// (llsm_gpu_batch_align_sub): the cells reached from some cell of row 0, ceil(i / 2) ... nb - 1; there is no upper cut.
__host__ __device__ static inline void align_sub_row(long long i, int nb, int& lo, int& hi) {
  lo = (int)((i + 1) / 2); hi = nb - 1;
}
// One pair: rows [a0, a0 + na) of code_a against rows [b0, b0 + nb) of code_b (flat frame indices); its plane -- [na][nb],
// or [na][2 band + 1] of a banded call -- starts at float cell0 of the planes, its moves at entry mv0 (`steps` entries of
// 16 bytes per strip of 64 rows: the anti-diagonals of the strip whose column window is the widest), its hand-over row
// (two rows of nb floats under the slope pattern) at float row0, its positions at float pos0 of the out block.  band is 0
// and not read where the whole matrix is searched.  pad is 0 except for llsm_gpu_batch_align_band_slope, where the pair's rows
// of the region (rule K1) start at entry pad of the table, and for llsm_gpu_batch_align_sub, where the pair's row of the
// matching function (rule Q4: nb floats) starts at float pad of the rows of all pairs.
struct AlignPair { int a0, na, b0, nb; int cell0, row0, pos0, band; long long mv0; int steps, pad; };
#define ALIGN_TILE 64                                  // k_align_dist_t: cells per side of a workgroup's tile
// The geometry of a row, which every kernel template is instantiated for: the whole matrix; the band of rule B1, whose
// centre is align_band_center; the band of rule A1, whose centre c_i of pair p is center[p.pos0 + i] of a device table (the
// pair's offset into pos is its offset into the concatenated centre lines): the last argument of the launchers, sum of na
// ints, read under ALIGN_GEO_LINE alone.  It is an argument of its own behind the others, not a member of AlignDev, so
// that the kernels of the other two geometries keep their argument layout and with it their machine code.
enum AlignGeo { ALIGN_GEO_FULL = 0, ALIGN_GEO_BAND = 1, ALIGN_GEO_LINE = 2 };
struct AlignDev {
  const float* code_a; const float* code_b; int dim, first, count; float step_cost, voicing_cost;
  const AlignPair* pairs; int n_pairs;
};
// D1 / B2: tiles[t] = (pair, first row, first column -- which may be negative in a band --, 0) of tile t; the planes of all
// pairs in one launch, under a band geometry in the band layout, every entry written, +infinity where its column lies outside
// the matrix
int launch_align_dist(LaunchCtx* P, AlignGeo geo, const AlignDev& d, const int4* tiles, int n_tiles, float* plane, const int* center);
// D2 - D3 / B3 - B4 over the planes, one wavefront per pair: out[pair.pos0 + i] = pos[i], out[cost0 + p] = cost of pair p
int launch_align_dtw(LaunchCtx* P, AlignGeo geo, const AlignDev& d, const float* plane, uint4* moves, float* row, float* out, int cost0,
  const int* center);
// L3 - L4 over whole-matrix planes or, under a band geometry, K3 - K4 over band planes, one wavefront per pair; region (read
// under a band geometry alone): {lo, hi} of every row of every pair (an empty row: lo > hi), pair p's from entry
// pairs[p].pad; row: two hand-over rows of nb floats per pair, out as above
int launch_align_slope_dtw(LaunchCtx* P, AlignGeo geo, const AlignDev& d, const float* plane, const int2* region, uint4* moves,
  float* row, float* out, int cost0, const int* center);
// Q3 - Q5 over whole-matrix planes (llsm_gpu_batch_align_sub), one wavefront per pair: the path kernels above with free
// ends, D2's moves or with `slope` L3's over the rows of Q1; row and out as above (two hand-over rows under the pattern),
// last_rows: acc of the last row of every pair, pair p's nb floats from float pairs[p].pad, +infinity left of the row's
// range; span[2 p], span[2 p + 1]: the first and the last column of pair p's path
int launch_align_sub_dtw(LaunchCtx* P, bool slope, const AlignDev& d, const float* plane, uint4* moves, float* row, float* out, int cost0,
  float* last_rows, int* span);
// P1 (llsm_gpu_batch_pool_code, llsm_gpu_batch_align_pyramid): the means of every `factor` (1 ... 64) consecutive rows of
// CODE, the last group of an utterance over the rows it has.  tab[u] = (first source frame, frames, first coarse frame of
// out, side: 0 reads code_a, 1 code_b) of pooled utterance u, n_tab >= 1 of them, the third member ascending from 0 and each
// utterance ceil(frames / factor) coarse frames long; out: [coarse_frames][dim]
int launch_pool_code(LaunchCtx* P, const float* code_a, const float* code_b, const int4* tab, int n_tab, int dim, int factor,
  long long coarse_frames, float* out);

// ---- unit selection (select.cpp, select_kernels.hip; rules S1 - S5 and C1 - C6: llsm_gpu.h)
#define SELECT_K 8                                     // candidates kept per target frame
#define SELECT_SEG 1024                                // k_select_knn: bank frames per segment at the least ...
#define SELECT_MAX_SEG 64                              // ... and segments at the most (one lane each in k_select_merge)
// the segment rule, of the bank's frames n alone: the bank is cut into min(64, ceil(n / 1024)) parts, a part rounded up to
// a multiple of 64 frames is the segment length, and the segments are as many of that length as cover the bank
static inline int select_seg_len(int n) {
  int s = (n + SELECT_SEG - 1) / SELECT_SEG; s = s < 1 ? 1 : s > SELECT_MAX_SEG ? SELECT_MAX_SEG : s;
  return (int)((((long long)n + s - 1) / s + 63) / 64 * 64);
}
static inline int select_segments(int n) { const int l = select_seg_len(n); const int s = (n + l - 1) / l; return s < 1 ? 1 : s; }
struct SelectDev {
  const float* code_t; const float* code_b; int dim, first, count;      // rows of t and of the bank
  float voicing_cost, join_cost, join_weight; int skip_own;
  int nt, nb, n_utt;                                                      // frames of t, frames of the bank, utterances of t
  const int* t_frm_off; const int* t_nfrm; const int* t_frm_utt;          // t: per utterance, per utterance, per frame
  const int* b_frm_off; const int* b_nfrm; const int* b_frm_utt;          // the bank likewise
  int n_seg, seg_len;
};
// S1 - S2 per bank segment: lists[seg][nt][16] (n_seg == 1: plane 7 itself)
int launch_select_knn(LaunchCtx* P, const SelectDev& d, float* lists);
// the K lowest of the n_seg lists of every target frame -> plane 7 [nt][16]
int launch_select_merge(LaunchCtx* P, const SelectDev& d, const float* lists, float* p7);
// S3: plane 8 [nt][64] from plane 7
int launch_select_join(LaunchCtx* P, const SelectDev& d, const float* p7, float* p8);
// S4 - S5, one wavefront per utterance of t: out = [utt of every frame | pos of every frame (float bits) | cost per utterance (float bits)]
int launch_select_path(LaunchCtx* P, const SelectDev& d, const float* p7, const float* p8, uint2* bp, int* out);
// C2 - C6 (llsm_gpu_batch_select_chain), one wavefront per utterance of t: near [nt][16] in the layout of plane 7 -> plane 10
// [nt][32], plane 11 [nt][256], one word of back pointers per frame, and out as launch_select_path gives it
#define SELECT_STATES 16                               // states per frame: SELECT_K near slots and up to SELECT_K followers
int launch_select_chain(LaunchCtx* P, const SelectDev& d, const float* near, float* p10, float* p11, uint2* bp, int* out);

#endif
