// modify_kernels.hip -- edits of a device-resident batch between analysis and synthesis (host side: modify.cpp).
//
//   k_phase_shift   llsm_frame_phaseshift on the rows of every frame (model.cpp), with the shift either given per frame
//                   or formed from the frame's reference phase (llsm_frame_phasesync_rps); one wavefront per frame
//   k_prop_theta    the per-frame shifts of llsm_chunk_phasepropagate: float32 running sum of an utterance's F0 row, in
//                   frame order, staged through LDS; one workgroup per utterance
//   k_pitch_formant F0 scaling, VTMAGN amplitude compensation and formant warp (VTMAGN, optionally PSD) of
//                   llsm_gpu_batch_pitch_formant; four consecutive frames per 256-thread workgroup, rows staged in LDS with
//                   16-byte accesses, the warp a gather from LDS
//   k_splice        llsm_gpu_batch_retime and llsm_gpu_batch_splice: the frame-blending step of the reference's time-stretch
//                   recipe as a pair rule P(A, B, r) on two frames; every output frame is P applied to two frames that are
//                   themselves P of two frames of any utterance of another batch (retime: one side, the frame's own
//                   utterance); four consecutive output frames per 256-thread workgroup, 16-byte stores, 16-byte loads at
//                   the source's own alignment, only the frames' scalars in LDS
//   k_smooth_rows   llsm_gpu_batch_smooth, first half: the triangular float64 means of F0, RD, VTMAGN, PSD and EDC of a tile
//                   of up to 16 consecutive frames into scratch rows; a thread owns a column, walks the tile's source frames
//                   once in ascending order and adds each value into the register accumulators of the outputs whose window
//                   holds the frame
//   k_smooth_store  second half, behind it on the stream: the scratch rows back into the batch, 16-byte stores where the
//                   span allows, NHAR = HAS_HM = 0 on smoothed voiced frames
//
// No `#pragma clang fp contract(fast)` here: the phase kernels reproduce the host's float64 arithmetic bit for bit and the
// blends are x_a + (x_b - x_a) r without contraction (the library is built with -ffp-contract=off).
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "launch.h"
#include "plan.h"

namespace lp = llsm_plan;

#include "synth_frame.h"                                  // xcd_frame

namespace {
const int kPropChunk = 2048;                              // F0 values staged in LDS per pass of k_prop_theta

DEV int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// model.cpp wrap_phase: to (-pi, pi], float64, rounded to float
DEV float md_wrap(double x) {
  const double pi = 3.14159265358979323846;
  double y = x - 2.0 * pi * floor((x + pi) / (2.0 * pi));
  if(y <= -pi) y += 2.0 * pi;
  return (float)y;
}
// llsm_hmframe_phaseshift on the first n entries of one row
DEV void shift_row(float* p, int n, double th, int lane) {
  for(int k = lane; k < n; k += 64) p[k] = md_wrap((double)p[k] + th * ((double)k + 1.0));
}

DEV float lin(float a, float b, float r) { return a + (b - a) * r; }
DEV float circ(float pa, float pb, float r) {
  return atan2f(lin(sinf(pa), sinf(pb), r), lin(cosf(pa), cosf(pb), r));
}
// per-element pieces of the pair rule: the -80 dB floor of VTMAGN and the fade of the voiced side of a voicing change by the
// weight w
DEV float floor80(float x) { return fmaxf(x, -80.0f); }
DEV float fade_db(float w) { return 20.0f * log10f(fmaxf(1e-8f, w)); }

// k_pitch_formant: a workgroup takes frames g0 .. g0 + 3 with g0 a multiple of 4, so its spans of VTMAGN (4 nspec floats)
// and PSD (4 npsd floats) start on a 16-byte boundary of the (256-byte aligned) rows and move as float4; only the batch's
// last group can end off a float4 and finish with single floats.
const int kPfFrames = 4, kPfThreads = 256;

// bin k of row x (n bins) warped by alpha: the envelope at f moves to alpha f (llsm_gpu.h)
DEV float warp_at(const float* x, int n, double alpha, int k) {
  const double p = (double)k / alpha;
  if(p >= (double)(n - 1)) return x[n - 1];              // floor(p) >= n - 1: the top bin is held
  const int i = (int)p;                                   // (p >= 0: truncation is floor)
  return lin(x[i], x[i + 1], (float)(p - (double)i));
}
// span [0, n) of global row memory <-> LDS, float4 where it can
DEV void pf_stage(float* __restrict__ d, const float* __restrict__ s, int n, int tid) {
  const int n4 = n >> 2;
  for(int q = tid; q < n4; q += kPfThreads) ((float4*)d)[q] = ((const float4*)s)[q];
  for(int e = (n4 << 2) + tid; e < n; e += kPfThreads) d[e] = s[e];
}
// k_splice: a workgroup takes output frames g0 .. g0 + 3 with g0 a multiple of 4 (k_pitch_formant's shape), so its spans
// of VTMAGN, PSD, PSDRES, AMPL, PHSE and VSPHSE start on a 16-byte boundary and are stored as float4.  The source rows sit
// wherever their frame index leaves them: they are read 16 bytes at float alignment (k_blob_pack's F4U), and as single
// floats where four output elements straddle two frames.
const int kSpFrames = 4, kSpThreads = 256;

struct __attribute__((packed, aligned(4))) SpF4U { float x, y, z, w; };     // 16 bytes at float alignment
template <int N> struct SpVec { float v[N]; };
// circ as ONE function of k_splice: inlined at each of its uses (both levels, both row kinds, both widths) the kernel was
// 126 KB of code, twice the instruction cache; the arithmetic and its bits are those of circ
__device__ __attribute__((noinline)) float sp_circ(float pa, float pb, float r) { return circ(pa, pb, r); }
template <int N> DEV SpVec<N> sp_ld(const float* p);
template <> DEV SpVec<1> sp_ld<1>(const float* p) { SpVec<1> o; o.v[0] = p[0]; return o; }
template <> DEV SpVec<4> sp_ld<4>(const float* p) {
  const SpF4U t = *(const SpF4U*)p;
  SpVec<4> o; o.v[0] = t.x; o.v[1] = t.y; o.v[2] = t.z; o.v[3] = t.w; return o;
}

// the scalars of one frame, stored or blended
struct SpScal { float f0, rd; int nv, ne, nhar, has_hm, pbpsyn; };
DEV SpScal sp_scal(const ModRows& s, size_t g) {
  SpScal o;
  o.f0 = s.f0[g]; o.rd = s.rd[g]; o.nv = s.nvsphse[g]; o.ne = s.nhar_e[g]; o.nhar = s.nhar[g]; o.has_hm = s.has_hm[g];
  o.pbpsyn = s.pbpsyn[g];
  return o;
}
// The pair rule P(A, B, r) (llsm_gpu.h) as one plan per frame pair: which case applies and the counts
// its rows need.  r == 0 is A and r == 1 is B, bit for bit.  Otherwise: both voiced (SP_VV): F0, RD and VTMAGN lin, VSPHSE circ
// over the shorter row, the rest from the longer; one voiced (SP_VU: A is, SP_UV: B is): that frame's F0, RD and VSPHSE, its
// VTMAGN faded by its weight; neither (SP_UU): F0 = 0, RD = 1, A's layer-1 rows.  PSD and EDC lin; the envelopes lin / circ over
// the shorter count, the rest from the longer.  A voiced output frame has no harmonic model (NHAR = HAS_HM = 0, zero rows:
// llsm_gpu_batch_tolayer0(dst, 1) rebuilds it from layer 1), an unvoiced one keeps A's.  PSDRES is not blended (SpFrame::gr).
enum { SP_COPY_A, SP_COPY_B, SP_VV, SP_VU, SP_UV, SP_UU };
struct SpPair { int mode; float r, fade; int nvmin, vlong, nemin, elong; };   // vlong / elong: the longer row is B's
// plan and resulting scalars of P(A, B, r) (B is not looked at when r == 0, nor A when r == 1)
DEV void sp_pair(const SpScal& A, const SpScal& B, float r, int mh, int mne, SpPair* p, SpScal* o) {
  p -> r = r; p -> fade = 0.0f; p -> nvmin = p -> vlong = p -> nemin = p -> elong = 0;
  if(r == 0.0f) { p -> mode = SP_COPY_A; *o = A; return; }
  if(r == 1.0f) { p -> mode = SP_COPY_B; *o = B; return; }
  const bool va = A.f0 > 0.0f, vb = B.f0 > 0.0f;
  const int nva = clampi(A.nv, 0, mh), nvb = clampi(B.nv, 0, mh);
  const int nea = clampi(A.ne, 0, mne), neb = clampi(B.ne, 0, mne);
  p -> nvmin = min(nva, nvb); p -> vlong = nva >= nvb ? 0 : 1;
  p -> nemin = min(nea, neb); p -> elong = nea >= neb ? 0 : 1;
  if(va && vb) {
    p -> mode = SP_VV; o -> f0 = lin(A.f0, B.f0, r); o -> rd = lin(A.rd, B.rd, r); o -> nv = max(nva, nvb);
  } else if(va || vb) {
    p -> mode = va ? SP_VU : SP_UV; p -> fade = fade_db(va ? 1.0f - r : r);
    o -> f0 = va ? A.f0 : B.f0; o -> rd = va ? A.rd : B.rd; o -> nv = va ? nva : nvb;
  } else {
    p -> mode = SP_UU; o -> f0 = 0.0f; o -> rd = 1.0f; o -> nv = nva;
  }
  const bool voiced = va || vb;
  o -> ne = max(nea, neb); o -> pbpsyn = A.pbpsyn;
  o -> nhar = voiced ? 0 : A.nhar; o -> has_hm = voiced ? 0 : A.has_hm;
}

// the kinds of rows: VTMAGN; VSPHSE; PSD and EDC; EENV_AMPL; EENV_PHSE; AMPL and PHSE; PSDRES
enum { SP_VT, SP_VS, SP_LIN, SP_EA, SP_EP, SP_HM, SP_RES };
template <int ROW> DEV bool sp_needs_a(int m) {
  if(ROW == SP_VT || ROW == SP_VS) return m != SP_COPY_B && m != SP_UV;
  if(ROW == SP_HM) return m == SP_COPY_A || m == SP_UU;
  return m != SP_COPY_B;
}
template <int ROW> DEV bool sp_needs_b(int m) {
  if(ROW == SP_VT || ROW == SP_VS) return m == SP_COPY_B || m == SP_VV || m == SP_UV;
  if(ROW == SP_HM) return m == SP_COPY_B;
  return m != SP_COPY_A;
}
// elements k .. k + N - 1 of a row of kind ROW of P(A, B, r); la() / lb() give the two frames' elements and are called only
// where the case reads that frame
template <int N, int ROW, class LA, class LB>
DEV SpVec<N> sp_blend(const SpPair& p, int k, int me, LA la, LB lb) {
  SpVec<N> a = {}, b = {}, o;
  const int m = p.mode;
  if(sp_needs_a<ROW>(m)) a = la();
  if(sp_needs_b<ROW>(m)) b = lb();
  if(m == SP_COPY_A) return a;
  if(m == SP_COPY_B) return b;
  const float r = p.r;
#pragma unroll
  for(int j = 0; j < N; j ++) {
    const float xa = a.v[j], xb = b.v[j];
    float y;
    if(ROW == SP_VT) y = floor80(m == SP_VV ? lin(xa, xb, r) : (m == SP_VU ? xa + p.fade : (m == SP_UV ? xb + p.fade : xa)));
    else if(ROW == SP_VS) {
      if(m == SP_VV) y = k + j < p.nvmin ? sp_circ(xa, xb, r) : (p.vlong ? xb : xa);
      else y = m == SP_UV ? xb : xa;
    }
    else if(ROW == SP_LIN) y = lin(xa, xb, r);
    else if(ROW == SP_EA) y = (k + j) % me < p.nemin ? lin(xa, xb, r) : (p.elong ? xb : xa);
    else if(ROW == SP_EP) y = (k + j) % me < p.nemin ? sp_circ(xa, xb, r) : (p.elong ? xb : xa);
    else y = m == SP_UU ? xa : 0.0f;                       // SP_HM: voiced output frames get zero rows
    o.v[j] = y;
  }
  return o;
}

// one output frame of k_splice: sides A and B are P of source frames ga, ga + 1 and gb, gb + 1, the output P(A, B, mix);
// gr: the source frame of its PSDRES row
struct SpFrame { SpPair o, a, b; int ga, gb, gr; };
template <int N, int ROW>
DEV SpVec<N> sp_el(const SpFrame& F, const float* __restrict__ s, int W, int k, int me) {
  if(ROW == SP_RES) return sp_ld<N>(s + (size_t)F.gr * W + k);
  auto side = [&](const SpPair& p, int g) {
    const float* x = s + (size_t)g * W + k;
    return sp_blend<N, ROW>(p, k, me, [&] { return sp_ld<N>(x); }, [&] { return sp_ld<N>(x + W); });
  };
  return sp_blend<N, ROW>(F.o, k, me, [&] { return side(F.a, F.ga); }, [&] { return side(F.b, F.gb); });
}
// the span of one kind of row (W floats per frame) of the workgroup's nf frames, from source array s into d
template <int ROW, bool VEC>
DEV void sp_span(float* __restrict__ d, const float* __restrict__ s, int W, int nf, const SpFrame* F, int me, int tid) {
  const int n = nf * W, n4 = VEC ? n >> 2 : 0;
  for(int q = tid; q < n4; q += kSpThreads) {
    int f = (4 * q) / W, k = 4 * q - f * W;
    SpVec<4> o;
    if(k + 4 <= W) o = sp_el<4, ROW>(F[f], s, W, k, me);
    else for(int j = 0; j < 4; j ++) { o.v[j] = sp_el<1, ROW>(F[f], s, W, k, me).v[0]; if(++ k == W) { k = 0; f ++; } }
    ((float4*)d)[q] = make_float4(o.v[0], o.v[1], o.v[2], o.v[3]);
  }
  for(int e = (n4 << 2) + tid; e < n; e += kSpThreads) { const int f = e / W; d[e] = sp_el<1, ROW>(F[f], s, W, e - f * W, me).v[0]; }
}
}  // namespace

__global__ __launch_bounds__(64) void k_phase_shift(ModRows r, const float* __restrict__ theta, int layer1_based) {
  const int g = xcd_frame(blockIdx.x, gridDim.x), lane = threadIdx.x;
  const size_t G = (size_t)g;
  const int me = r.maxnhar_e > 0 ? r.maxnhar_e : 1;
  // counts as the rows define them: HM and noise envelopes only on voiced frames (llsm_flat_to_chunk), HM only where
  // HAS_HM says it is valid, VSPHSE on frames with layer-1 members
  const bool voiced = r.f0[g] != 0.0f;
  const bool hm = voiced && (r.has_hm == nullptr || r.has_hm[g] != 0);
  const int nh = hm ? clampi(r.nhar[g], 0, r.maxnhar) : 0;
  const int ne = voiced ? clampi(r.nhar_e[g], 0, r.maxnhar_e) : 0;
  const int nv = r.nvsphse ? clampi(r.nvsphse[g], 0, r.maxnhar) : 0;
  float th;
  if(theta) th = theta[g];
  else {                                                  // llsm_frame_phasesync_rps
    float ref = 0;
    if(layer1_based && nv > 0) ref = r.vsphse[G * r.maxnhar];
    else if(nh > 0) ref = r.phse[G * r.maxnhar];
    th = -ref;
  }
  const double t = (double)th;
  shift_row(r.phse + G * r.maxnhar, nh, t, lane);
  for(int c = 0; c < r.nchannel; c ++) shift_row(r.eenv_phse + (G * r.nchannel + c) * me, ne, t, lane);
  if(nv > 0) shift_row(r.vsphse + G * r.maxnhar, nv, t, lane);
}

__global__ __launch_bounds__(256) void k_prop_theta(const int* __restrict__ frm_off, const int* __restrict__ nfrm,
  const float* __restrict__ f0, double k2pi, float* __restrict__ theta) {
  __shared__ float buf[kPropChunk];
  const int u = blockIdx.x, tid = threadIdx.x;
  const int off = frm_off[u], n = nfrm[u];
  float acc = 0;                                          // (thread 0's is the running sum)
  for(int c0 = 0; c0 < n; c0 += kPropChunk) {
    const int m = min(kPropChunk, n - c0);
    for(int i = tid; i < m; i += 256) buf[i] = f0[off + c0 + i];
    __syncthreads();
    if(tid == 0)
      for(int i = 0; i < m; i ++) { acc += buf[i]; buf[i] = (float)((double)acc * k2pi); }
    __syncthreads();
    for(int i = tid; i < m; i += 256) theta[off + c0 + i] = buf[i];
    __syncthreads();
  }
}

// Thread (f, j) of the first sixteen fetches the scalars of source frame j (a, a + 1 of side A; a, a + 1 of side B) of output
// frame f where the map makes the frame read it; thread f then plans the frame and writes its scalars.
__global__ __launch_bounds__(kSpThreads) void k_splice(ModRows s, ModRows d, SpliceMap m) {
  __shared__ SpScal s_src[kSpFrames][4];
  __shared__ SpFrame s_frm[kSpFrames];
  const int g0 = xcd_frame(blockIdx.x, gridDim.x) * kSpFrames, tid = threadIdx.x;
  const int nf = min(kSpFrames, d.nframes - g0);
  const int mh = s.maxnhar, np = s.npsd, nch = s.nchannel, ns = s.nspec;
  const int me = s.maxnhar_e > 0 ? s.maxnhar_e : 1;
  if(tid < 4 * nf) {
    const int g = g0 + (tid >> 2), j = tid & 3;
    const float mix = m.mix ? m.mix[g] : 0.0f;
    const bool side_b = j >= 2;
    if(side_b ? mix != 0.0f : mix != 1.0f) {               // (a side the output does not use is not read)
      const float r = side_b ? m.rb[g] : m.ra[g];
      if(j & 1 ? r != 0.0f : r != 1.0f) s_src[tid >> 2][j] = sp_scal(s, (size_t)(side_b ? m.gb[g] : m.ga[g]) + (j & 1));
    }
  }
  __syncthreads();
  if(tid < nf) {
    const int g = g0 + tid;
    SpFrame F;
    const float mix = m.mix ? m.mix[g] : 0.0f;
    SpScal A = {}, B = {}, O;
    F.ga = m.ga[g]; F.gb = m.mix ? m.gb[g] : 0;
    F.a.mode = F.b.mode = SP_COPY_A;
    float ra = 0.0f, rb = 0.0f;
    if(mix != 1.0f) { ra = m.ra[g]; sp_pair(s_src[tid][0], s_src[tid][1], ra, mh, s.maxnhar_e, & F.a, & A); }
    if(mix != 0.0f) { rb = m.rb[g]; sp_pair(s_src[tid][2], s_src[tid][3], rb, mh, s.maxnhar_e, & F.b, & B); }
    sp_pair(A, B, mix, mh, s.maxnhar_e, & F.o, & O);
    // PSDRES: the map's frame; without one the frame at floor(pos) of side A below mix 0.5, of side B from there on (r == 1
    // only at an utterance's end)
    F.gr = m.gr ? m.gr[g] : (mix < 0.5f ? F.ga + (ra == 1.0f) : F.gb + (rb == 1.0f));
    s_frm[tid] = F;
    d.f0[g] = O.f0; d.rd[g] = O.rd; d.nvsphse[g] = O.nv; d.nhar_e[g] = O.ne; d.nhar[g] = O.nhar; d.has_hm[g] = O.has_hm;
    d.pbpsyn[g] = O.pbpsyn; d.has_psdres[g] = s.has_psdres[F.gr];
  }
  __syncthreads();
  const size_t G0 = (size_t)g0;
  sp_span<SP_VT, true>(d.vtmagn + G0 * ns, s.vtmagn, ns, nf, s_frm, me, tid);
  sp_span<SP_LIN, true>(d.psd + G0 * np, s.psd, np, nf, s_frm, me, tid);
  sp_span<SP_RES, true>(d.psdres + G0 * np, s.psdres, np, nf, s_frm, me, tid);
  sp_span<SP_VS, true>(d.vsphse + G0 * mh, s.vsphse, mh, nf, s_frm, me, tid);
  sp_span<SP_HM, true>(d.ampl + G0 * mh, s.ampl, mh, nf, s_frm, me, tid);
  sp_span<SP_HM, true>(d.phse + G0 * mh, s.phse, mh, nf, s_frm, me, tid);
  sp_span<SP_LIN, false>(d.edc + G0 * nch, s.edc, nch, nf, s_frm, me, tid);
  sp_span<SP_EA, false>(d.eenv_ampl + G0 * nch * me, s.eenv_ampl, nch * me, nf, s_frm, me, tid);
  sp_span<SP_EP, false>(d.eenv_phse + G0 * nch * me, s.eenv_phse, nch * me, nf, s_frm, me, tid);
}

// The span of VTMAGN (ns bins per frame) or PSD of one workgroup's frames, rewritten from its LDS image `x`: bin k of local
// frame f is warped by alpha[f] where warp[f], minus comp[f] where sub[f] (sub NULL: nowhere), and copied otherwise.
DEV void pf_write(float* __restrict__ d, const float* __restrict__ x, int ns, int nf, const int* warp, const int* sub,
  const float* alpha, const double* comp, int tid) {
  auto val = [&](int f, int k) {
    const float* xf = x + f * ns;
    const bool s = sub && sub[f];
    if(! warp[f] && ! s) return xf[k];
    const float w = warp[f] ? warp_at(xf, ns, (double)alpha[f], k) : xf[k];
    return s ? (float)((double)w - comp[f]) : w;
  };
  const int n = nf * ns, n4 = n >> 2;
  for(int q = tid; q < n4; q += kPfThreads) {
    int f = (4 * q) / ns, k = 4 * q - f * ns;
    float o[4];
    for(int j = 0; j < 4; j ++) { o[j] = val(f, k); if(++ k == ns) { k = 0; f ++; } }
    ((float4*)d)[q] = make_float4(o[0], o[1], o[2], o[3]);
  }
  for(int e = (n4 << 2) + tid; e < n; e += kPfThreads) d[e] = val(e / ns, e % ns);
}

// g_lo: first frame of the launch (a multiple of kPfFrames); frames whose two ratios are both 1 are left alone
__global__ __launch_bounds__(kPfThreads) void k_pitch_formant(ModRows r, int g_lo, const float* __restrict__ rho,
  const float* __restrict__ alpha, int warp_psd) {
  extern __shared__ float4 pf_lds[];
  __shared__ int s_vt[kPfFrames], s_psd[kPfFrames], s_warpvt[kPfFrames];
  __shared__ float s_alpha[kPfFrames];
  __shared__ double s_comp[kPfFrames];
  const int g0 = g_lo + (int)blockIdx.x * kPfFrames, tid = threadIdx.x;
  const int nf = min(kPfFrames, r.nframes - g0);
  // the ratios first: a group with nothing to do ends here, before it reads a row
  bool any = false;
  for(int f = 0; f < nf; f ++) any = any || (rho ? rho[g0 + f] : 1.0f) != 1.0f || (alpha ? alpha[g0 + f] : 1.0f) != 1.0f;
  if(! any) return;
  if(tid < kPfFrames) {
    int vt = 0, ps = 0; float al = 1.0f; double comp = 0.0;
    if(tid < nf) {
      const int g = g0 + tid;
      const float rh = rho ? rho[g] : 1.0f;
      al = alpha ? alpha[g] : 1.0f;
      const bool touched = rh != 1.0f || al != 1.0f;
      const float f0 = r.f0[g];
      vt = touched && f0 != 0.0f;
      ps = warp_psd && al != 1.0f;
      if(vt) {
        comp = 20.0 * log10((double)rh);
        r.f0[g] = f0 * rh; r.nhar[g] = 0; r.has_hm[g] = 0;
      }
    }
    s_vt[tid] = vt; s_warpvt[tid] = vt && al != 1.0f; s_psd[tid] = ps; s_alpha[tid] = al; s_comp[tid] = comp;
  }
  __syncthreads();
  bool do_vt = false, do_psd = false;
  for(int f = 0; f < nf; f ++) { do_vt = do_vt || s_vt[f]; do_psd = do_psd || s_psd[f]; }
  const int ns = r.nspec, np = r.npsd;
  float* lv = (float*)pf_lds;                             // [kPfFrames][ns] VTMAGN, then [kPfFrames][np] PSD
  float* lp_ = lv + kPfFrames * ns;
  float* gv = r.vtmagn + (size_t)g0 * ns;
  float* gp = r.psd + (size_t)g0 * np;
  if(do_vt) pf_stage(lv, gv, nf * ns, tid);
  if(do_psd) pf_stage(lp_, gp, nf * np, tid);
  __syncthreads();
  if(do_vt) pf_write(gv, lv, ns, nf, s_warpvt, s_vt, s_alpha, s_comp, tid);
  if(do_psd) pf_write(gp, lp_, np, nf, s_psd, nullptr, s_alpha, s_comp, tid);
}

// ---- llsm_gpu_batch_smooth (rules S1 - S9 of llsm_gpu.h)
namespace {
const int kSmThreads = 256;
const int kSmReach = kSmoothTile + 2 * kSmoothMaxRadius;  // frames whose voicing the windows of one tile may ask for

// one frame of a tile as its threads share it: the window [lo, hi] of rule S2 and R + 1 in one word -- lo and hi counted
// from the first frame of the tile's reach, bits 0 - 7 and 8 - 15, R + 1 in bits 16 - 23 --, the sum of the weights and the
// mark the store goes by (0: rule S3 or no frame, 1: unvoiced, 2: voiced)
struct SmFrame { int win, wsum, mark; };
const int kSmNoWindow = 0xff;                             // lo = 255 > hi = 0: holds no frame
DEV int sm_reach0(const SmoothTile& t) { return max(t.u0, t.g0 - kSmoothMaxRadius); }

// The frames of tile t planned from the F0 row: the F0 values within the tile's reach come into LDS once, then thread f
// shrinks the window of frame f to its voicing run.  Entries f >= t.cnt get no window.
DEV void sm_plan(const ModRows& r, const SmoothTile& t, const int* __restrict__ radius, float* s_f0, SmFrame* s_frm, int tid) {
  const int b0 = sm_reach0(t), b1 = min(t.u1, t.g0 + t.cnt - 1 + kSmoothMaxRadius);
  for(int q = tid; q <= b1 - b0; q += kSmThreads) s_f0[q] = r.f0[b0 + q];       // (at most kSmReach values)
  __syncthreads();
  if(tid < kSmoothTile) {
    SmFrame F = {kSmNoWindow, 1, 0};
    if(tid < t.cnt) {
      const int g = t.g0 + tid, R = radius[t.slot + tid];
      const bool v = s_f0[g - b0] != 0.0f;
      const int wlo = max(t.u0, g - R), whi = min(t.u1, g + R);
      int lo = g, hi = g;
      while(lo > wlo && (s_f0[lo - 1 - b0] != 0.0f) == v) lo --;
      while(hi < whi && (s_f0[hi + 1 - b0] != 0.0f) == v) hi ++;
      int wsum = 0;
      for(int j = lo; j <= hi; j ++) wsum += R + 1 - abs(j - g);
      F.win = (lo - b0) | (hi - b0) << 8 | (R + 1) << 16; F.wsum = wsum; F.mark = lo == hi ? 0 : (v ? 2 : 1);
    }
    s_frm[tid] = F;
  }
  __syncthreads();
}

// One track of the tile: `width` columns, element k of frame j of the reach (flat frame b0 + j) at x[j * stride + k], results
// into column k of the scratch rows at `out` (row_w floats apart).  want: the least mark that takes part (2: a track of
// voiced frames only).  c0: the tile's first frame, counted from b0.
// A thread owns column k: it walks the source frames from the tile's smallest lo to its largest hi once, ascending, loads
// x_j[k] once and adds w x into the float64 accumulator of every output whose window holds j -- so every output's additions
// come in ascending j (rule S4).  The windows are wave-uniform (one scalar register each), the accumulators registers
// indexed by the unrolled loops alone.
DEV void sm_track(const float* __restrict__ x, int stride, int width, int want, const SmFrame* s_frm, int c0,
  float* __restrict__ out, int row_w, int tid) {
  int win[kSmoothTile];
  int jmin = 0x7fffffff, jmax = -1;
#pragma unroll
  for(int f = 0; f < kSmoothTile; f ++) {
    win[f] = __builtin_amdgcn_readfirstlane(s_frm[f].mark >= want ? s_frm[f].win : kSmNoWindow);
    const int lo = win[f] & 0xff, hi = win[f] >> 8 & 0xff;
    if(lo <= hi) { jmin = min(jmin, lo); jmax = max(jmax, hi); }
  }
  if(jmax < 0) return;                                    // no frame of the tile takes part in this track
  const int lane = tid & 63;
  for(int k0 = tid - lane; k0 < width; k0 += kSmThreads) {
    const int k = k0 + lane;
    const bool live = k < width;
    double acc[kSmoothTile];
#pragma unroll
    for(int f = 0; f < kSmoothTile; f ++) acc[f] = 0.0;
    for(int j = jmin; j <= jmax; j ++) {
      const double xv = live ? (double)x[(size_t)j * stride + k] : 0.0;
#pragma unroll
      for(int f = 0; f < kSmoothTile; f ++) {
        int w = win[f];
        asm volatile("" : "+s"(w));                       // unpacked here, every time: hoisted out of the loop the three
                                                          // fields of sixteen windows spilled scalar registers
        if(j >= (w & 0xff) && j <= (w >> 8 & 0xff)) acc[f] = acc[f] + (double)((w >> 16) - abs(j - (c0 + f))) * xv;
      }
    }
    if(live) {
#pragma unroll
      for(int f = 0; f < kSmoothTile; f ++) {
        int w = win[f];
        asm volatile("" : "+s"(w));                       // (as above: sixteen conditions kept as lane masks spilled too)
        if((w & 0xff) <= (w >> 8 & 0xff)) out[(size_t)f * row_w + k] = (float)(acc[f] / (double)s_frm[f].wsum);
      }
    }
  }
}

// The span of one track (W floats per frame) of a tile's nf frames, from the scratch rows at `sc` (row_w floats apart) back
// into the batch's row at d; frames with ok[f] == 0 are left alone.  d starts wherever its frame index leaves it: single
// floats up to the first 16-byte boundary, then float4 where all four elements belong to frames that are written, single
// floats elsewhere and behind the last float4.
DEV void sm_span(float* __restrict__ d, const float* __restrict__ sc, int W, int row_w, int nf, const int* ok, int tid) {
  const int n = nf * W;
  const int head = min(n, (int)((4 - (((size_t)d >> 2) & 3)) & 3)), n4 = (n - head) >> 2;
  auto one = [&](int e) { const int f = e / W; if(ok[f]) d[e] = sc[(size_t)f * row_w + (e - f * W)]; };
  if(tid < head) one(tid);
  for(int q = tid; q < n4; q += kSmThreads) {
    const int e = head + 4 * q, f1 = (e + 3) / W;
    int f = e / W, k = e - f * W;
    bool all = true;
    for(int ff = f; ff <= f1; ff ++) all = all && ok[ff];
    if(all) {
      float o[4];
      for(int j = 0; j < 4; j ++) { o[j] = sc[(size_t)f * row_w + k]; if(++ k == W) { k = 0; f ++; } }
      *(float4*)(d + e) = make_float4(o[0], o[1], o[2], o[3]);
    } else for(int j = 0; j < 4; j ++) one(e + j);
  }
  for(int e = head + (n4 << 2) + tid; e < n; e += kSmThreads) one(e);
}
}  // namespace

// One workgroup per tile (blockIdx.x) and track (blockIdx.y: bit y of the flags; a track that is not flagged ends at once).
// Reads the batch, writes job.rows and job.mark only: the store runs behind it on the stream, so every mean is formed from
// the rows as they were before the call.  Every workgroup of a tile plans the same windows and writes the same marks.
__global__ __launch_bounds__(kSmThreads) void k_smooth_rows(ModRows r, SmoothJob job) {
  __shared__ float s_f0[kSmReach];
  __shared__ SmFrame s_frm[kSmoothTile];
  const int track = 1 << blockIdx.y;
  if(!(job.flags & track)) return;
  const SmoothTile t = job.tiles[blockIdx.x];
  const int tid = threadIdx.x;
  sm_plan(r, t, job.radius, s_f0, s_frm, tid);
  if(tid < t.cnt) job.mark[t.slot + tid] = s_frm[tid].mark;
  const int ns = r.nspec, np = r.npsd, nch = r.nchannel, row_w = ns + np + nch + 2;
  const float* x; int width, col;
  switch(track) {
    case SM_F0: x = r.f0; width = 1; col = ns + np + nch; break;
    case SM_RD: x = r.rd; width = 1; col = ns + np + nch + 1; break;
    case SM_VTMAGN: x = r.vtmagn; width = ns; col = 0; break;
    case SM_PSD: x = r.psd; width = np; col = ns; break;
    default: x = r.edc; width = nch; col = ns + np; break;
  }
  const int b0 = sm_reach0(t);
  sm_track(x + (size_t)b0 * width, width, width, track & (SM_PSD | SM_EDC) ? 1 : 2, s_frm, t.g0 - b0,
    job.rows + (size_t)t.slot * row_w + col, row_w, tid);
}

// One workgroup per tile, the same tiles.  Unflagged tracks and frames of mark 0 (rule S3) are skipped; a voiced frame with
// any of its three tracks smoothed loses its harmonic model (rule S5).
__global__ __launch_bounds__(kSmThreads) void k_smooth_store(ModRows r, SmoothJob job) {
  __shared__ int s_v[kSmoothTile], s_n[kSmoothTile];
  const SmoothTile t = job.tiles[blockIdx.x];
  const int tid = threadIdx.x;
  if(tid < kSmoothTile) {
    const int m = tid < t.cnt ? job.mark[t.slot + tid] : 0;
    s_v[tid] = m == 2; s_n[tid] = m != 0;
  }
  __syncthreads();
  const int ns = r.nspec, np = r.npsd, nch = r.nchannel, row_w = ns + np + nch + 2;
  const float* sc = job.rows + (size_t)t.slot * row_w;
  const size_t G0 = (size_t)t.g0;
  if(job.flags & SM_VTMAGN) sm_span(r.vtmagn + G0 * ns, sc, ns, row_w, t.cnt, s_v, tid);
  if(job.flags & SM_PSD) sm_span(r.psd + G0 * np, sc + ns, np, row_w, t.cnt, s_n, tid);
  if(job.flags & SM_EDC) sm_span(r.edc + G0 * nch, sc + ns + np, nch, row_w, t.cnt, s_n, tid);
  if(tid < t.cnt && s_v[tid]) {
    const float* row = sc + (size_t)tid * row_w + ns + np + nch;
    const size_t g = G0 + tid;
    if(job.flags & SM_F0) r.f0[g] = row[0];
    if(job.flags & SM_RD) r.rd[g] = row[1];
    if(job.flags & (SM_F0 | SM_RD | SM_VTMAGN)) { r.nhar[g] = 0; r.has_hm[g] = 0; }
  }
}

int launch_smooth_rows(LaunchCtx* P, const ModRows& r, const SmoothJob& job) {
  if(job.ntiles <= 0) return 0;
  LAUNCH("k_smooth_rows", k_smooth_rows, dim3(job.ntiles, 5), dim3(kSmThreads), 0, r, job);
  return 0;
}

int launch_smooth_store(LaunchCtx* P, const ModRows& r, const SmoothJob& job) {
  if(job.ntiles <= 0) return 0;
  LAUNCH("k_smooth_store", k_smooth_store, dim3(job.ntiles), dim3(kSmThreads), 0, r, job);
  return 0;
}

int launch_phase_shift(LaunchCtx* P, const ModRows& r, const float* theta, int layer1_based) {
  if(r.nframes <= 0) return 0;
  LAUNCH("k_phase_shift", k_phase_shift, dim3(r.nframes), dim3(64), 0, r, theta, layer1_based);
  return 0;
}

int launch_phase_propagate_theta(LaunchCtx* P, int n_utt, const int* frm_off, const int* nfrm, const float* f0,
  double k2pi, float* theta) {
  if(n_utt <= 0) return 0;
  LAUNCH("k_prop_theta", k_prop_theta, dim3(n_utt), dim3(256), 0, frm_off, nfrm, f0, k2pi, theta);
  return 0;
}

int launch_splice(LaunchCtx* P, const ModRows& src, const ModRows& dst, const SpliceMap& m) {
  if(dst.nframes <= 0) return 0;
  const int groups = (dst.nframes + kSpFrames - 1) / kSpFrames;
  LAUNCH("k_splice", k_splice, dim3(groups), dim3(kSpThreads), 0, src, dst, m);
  return 0;
}

int launch_pitch_formant(LaunchCtx* P, const ModRows& r, int g_lo, int g_hi, const float* rho, const float* alpha,
  int warp_psd) {
  if(g_hi <= g_lo) return 0;
  g_lo -= g_lo % kPfFrames;
  const size_t lds = (size_t)kPfFrames * (r.nspec + r.npsd) * sizeof(float);
  const hipError_t e = lds_opt_in((const void*)k_pitch_formant, lds);
  if(e != hipSuccess) return (int)e;
  const int groups = (g_hi - g_lo + kPfFrames - 1) / kPfFrames;
  LAUNCH("k_pitch_formant", k_pitch_formant, dim3(groups), dim3(kPfThreads), lds, r, g_lo, rho, alpha, warp_psd);
  return 0;
}
