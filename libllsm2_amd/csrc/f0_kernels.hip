// f0_kernels.hip -- F0 of a batch's waveforms: the estimator llsm_gpu_batch_estimate_f0 and the tracker
// llsm_gpu_batch_track_f0 (rules: llsm_gpu.h, DESIGN.md sections 21 and 22; host side: f0.cpp).  Four kernels:
//
//   k_f0_energy      sum of squares of every utterance, float64, in an order fixed by the utterance's length
//   k_f0_cmndf_wf    one wavefront per frame pair on the register-resident wavefront FFT (wave_fft.h): the YIN difference
//                    function through a cross-correlation, the cumulative-mean-normalised difference (CMNDF), then
//                    either the lag search and the parabolic fit -> one raw F0 per frame (estimator), or <, CAND = true>
//                    the up to seven lowest dips of the row -> one candidate row per frame (tracker)
//   k_f0_median      estimator: the median-of-5 pass over the raw row of each utterance
//   k_f0_viterbi     tracker: one wavefront per utterance, the minimum-cost path through the candidate rows -> F0
//
// k_f0_cmndf_wf, per frame with segment s[0, W + lmax) (zero-padded to N = 2^LOGN >= W + lmax):
//   the complex transform of z = a + j s, a = s[0, W), carries the spectra of both real sequences; they separate by
//   symmetry, A[k] = (Z[k] + conj Z[N-k]) / 2, S[k] = (Z[k] - conj Z[N-k]) / 2j.  C = conj(A) S is the spectrum of the
//   REAL cross-correlation r(tau) = sum_{n<W} s[n] s[n+tau], so C1 + j C2 of the two frames of a pair goes through one
//   inverse transform (its upper half follows from the lower by symmetry): three transforms per two frames.  N >= W + lmax
//   keeps the lags [0, lmax] free of circular overlap.
//   d(tau) = E(0) + E(tau) - 2 r(tau) is a small difference of large terms near a period, so everything but r is float64:
//   E(tau) = E(0) + sum_{j<tau} (s[j+W]^2 - s[j]^2) and the running sum of d are prefix sums, taken with each lane on a
//   contiguous chunk of lags (serial inside the chunk, one wavefront scan across chunks) from s and r staged in the LDS
//   the transforms have left.  The CMNDF row goes back to the LDS as float32, where the two ordered searches of the lag
//   are ballots over 64 lags at a time.
#include <hip/hip_runtime.h>
#include <algorithm>

#include "kernels.h"
#include "plan.h"

namespace lp = llsm_plan;

#include "dev_common.h"
#include "wave_fft.h"
#include "launch.h"

extern __shared__ __attribute__((aligned(16))) unsigned char g_lds[];

// ---------------------------------------------------------------- per-utterance sum of squares
#define F0_EN_NT 256
__global__ __launch_bounds__(F0_EN_NT) void k_f0_energy(const float* __restrict__ x, const int* __restrict__ x_off,
  const int* __restrict__ nx, double* __restrict__ uss) {
  __shared__ double part[F0_EN_NT];
  const int u = blockIdx.x, tid = threadIdx.x, n = nx[u];
  const float* xs = x + x_off[u];
  double acc = 0.0;
  for(int i = tid; i < n; i += F0_EN_NT) { const double v = (double)xs[i]; acc += v * v; }
  part[tid] = acc;
  __syncthreads();
  for(int h = F0_EN_NT / 2; h > 0; h >>= 1) {
    if(tid < h) part[tid] += part[tid + h];
    __syncthreads();
  }
  if(tid == 0) uss[u] = part[0];
}

// ---------------------------------------------------------------- difference function, CMNDF, lag
DEV double wave_sum_d(double v) {
#pragma unroll
  for(int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, WAVE);
  return v;
}
// sum of v over the lanes below this one
DEV double wave_scan_excl_d(double v, int lane) {
#pragma unroll
  for(int o = 1; o < WAVE; o <<= 1) { const double t = __shfl_up(v, o, WAVE); if(lane >= o) v += t; }
  const double up = __shfl_up(v, 1, WAVE);
  return lane == 0 ? 0.0 : up;
}

// Cross-lane reads without the LDS pipe (data-parallel primitives of the vector ALU; every lane must be active): lane l
// reads lane l ^ 1 or l ^ 2 (quad permutes), or the lane 4, 8 or 12 below it round its row of 16 lanes (row rotations).
#define DPP_XOR1 0xB1
#define DPP_XOR2 0x4E
#define DPP_ROR4 0x124
#define DPP_ROR8 0x128
#define DPP_ROR12 0x12C
template <int CTRL> DEV int dpp_i(int v) { return __builtin_amdgcn_update_dpp(v, v, CTRL, 0xF, 0xF, false); }
template <int CTRL> DEV float dpp_f(float v) { return __builtin_bit_cast(float, dpp_i<CTRL>(__builtin_bit_cast(int, v))); }
DEV float lane_f(float v, int l) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l)); }
// the least v of the wavefront, on every lane: within the rows of 16 by permutes and rotations (a minimum may meet a
// lane twice), then over the four rows
DEV float wave_min_f(float v) {
  v = fminf(v, dpp_f<DPP_XOR1>(v)); v = fminf(v, dpp_f<DPP_XOR2>(v));
  v = fminf(v, dpp_f<DPP_ROR4>(v)); v = fminf(v, dpp_f<DPP_ROR8>(v));
  return fminf(fminf(lane_f(v, 0), lane_f(v, 16)), fminf(lane_f(v, 32), lane_f(v, 48)));
}
DEV int wave_min_i(int v) {
  v = min(v, dpp_i<DPP_XOR1>(v)); v = min(v, dpp_i<DPP_XOR2>(v));
  v = min(v, dpp_i<DPP_ROR4>(v)); v = min(v, dpp_i<DPP_ROR8>(v));
  return min(min(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)),
             min(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}

#define F0_CB 4                                    // lags a lane looks at per group in the candidate search
// CAND: rule T1 of llsm_gpu_batch_track_f0 instead of rules 6 - 7 -- the candidate row of the frame into c.plane, raw
// not written
template <int LOGN, bool CAND>
__global__ __launch_bounds__(WAVE, (LOGN >= 12 ? 1 : 2)) void k_f0_cmndf_wf(F0Dev d, const double* __restrict__ uss,
  float* __restrict__ raw, float* __restrict__ cmndf, F0Cand c) {
  constexpr int N = 1 << LOGN, P = N / WAVE, H = P / 2;
  const int lane = threadIdx.x;
  float2* lds = (float2*)g_lds;
  WfTw<LOGN> tw; wf_init(tw, lane);
  const int W = d.W, lmax = d.lmax, lmin = d.lmin, L = W + lmax;       // L <= N, lmax < N / 2 (f0.cpp)
  // after the transforms their LDS holds r, then the CMNDF, of one frame at R[0, lmax] and its zero-padded segment at
  // S[0, N): lmax + 4 + N <= N / 2 + 3 + N floats, and the exchanges own more than 2 N
  float* R = (float*)g_lds; float* S = R + ((lmax + 4) & ~3);
  const int CH = ((lmax + WAVE) / WAVE) | 1;                          // lags per lane, odd: the lanes' strides spread over the banks
  const int t0 = min(lane * CH, lmax + 1), t1 = min(t0 + CH, lmax + 1);
  const int per = (d.npairs + gridDim.x - 1) / gridDim.x;
  for(int p = blockIdx.x * per; p < min(d.npairs, (blockIdx.x + 1) * per); p ++) {
    const int2 pr = d.pairs[p];
    const int g0 = pr.x; const bool two = pr.y >= 0;                  // (g0, g0 + 1) of one utterance, or its last frame alone
    const int u = d.frm_utt[g0], i0 = g0 - d.frm_off[u], nxu = d.nx[u];
    const float* xs = d.x + d.x_off[u];
    int base[2];
    base[0] = lp::center(i0, d.thop, d.fs) - W / 2;
    base[1] = lp::center(i0 + 1, d.thop, d.fs) - W / 2;
    float xr[P], xi[P];                                               // z, Z, then C1 + j C2, then N r1 and N r2
    float c1r[H + 1], c1i[H + 1];
#pragma unroll
    for(int e = 0; e < 2; e ++) {
      if(e == 1 && ! two) break;
      // (opaque copy of the lane: the masks t < W of the registers depend on neither pair nor frame, and hoisted out of
      // the loops they stay live across the transforms in SGPRs that spill)
      int ln = lane; asm volatile("" : "+v"(ln));
      const int lo = max(base[e], 0);
      const buf_t seg = buf_range(xs, lo, min(base[e] + L, nxu));     // zero outside the utterance and behind the segment
#pragma unroll
      for(int m = 0; m < P; m ++) xi[m] = ld_range(seg, base[e] + ln + WAVE * m - lo);
#pragma unroll
      for(int m = 0; m < P; m ++) xr[m] = ln + WAVE * m < W ? xi[m] : 0.0f;
      wave_fft<LOGN>(xr, xi, tw, lds, lane);
      float mr[H + 1], mi[H + 1];
      wave_mirror_lo<P>(xr, mr, lane);
      wave_mirror_lo<P>(xi, mi, lane);
#pragma unroll
      for(int m = 0; m <= H; m ++) {
        const float ar = 0.5f * (xr[m] + mr[m]), ai = 0.5f * (xi[m] - mi[m]);      // A
        const float sr = 0.5f * (xi[m] + mi[m]), si = -0.5f * (xr[m] - mr[m]);     // S
        const float cr = ar * sr + ai * si, ci = ar * si - ai * sr;                // conj(A) S
        if(e == 0) { c1r[m] = cr; c1i[m] = ci; }
        else if(m < H) {
          // lower half: C1 + j C2; what the mirrored bin takes, conj C1 + j conj C2, waits in (mr, mi)
          xr[m] = c1r[m] - ci; xi[m] = c1i[m] + cr; mr[m] = c1r[m] + ci; mi[m] = cr - c1i[m];
        } else { xr[H] = c1r[H]; xi[H] = cr; }                        // Nyquist bin (lane 0; the other lanes are reflected into)
      }
      if(e == 1) { wave_reflect<P>(mr, xr, lane); wave_reflect<P>(mi, xi, lane); }
    }
    if(! two) {                                                        // a lone frame: C2 = 0
      float vi[H + 1];
#pragma unroll
      for(int m = 0; m < H; m ++) { xr[m] = c1r[m]; xi[m] = c1i[m]; vi[m] = -c1i[m]; }
      xr[H] = c1r[H]; xi[H] = 0.0f; vi[H] = 0.0f;
      wave_reflect<P>(c1r, xr, lane); wave_reflect<P>(vi, xi, lane);
    }
    wave_fft<LOGN>(xi, xr, tw, lds, lane);                            // inverse (x N): r1 in xr, r2 in xi
    // CAND: lane 8 e + k keeps candidate k of frame e -- its lag and the three CMNDF values around it -- until both frames
    // are through: the float64 of rule 7 and of the logarithm then has the registers of the transforms to itself
    int c_tau = 0; float c_y0 = 0.0f, c_y1 = 0.0f, c_y2 = 0.0f; bool c_have = false;

#pragma unroll
    for(int e = 0; e < 2; e ++) {
      if(e == 1 && ! two) break;
      const int g = g0 + e;
      // r and the segment into the LDS (the loads beyond the segment return zero: S[L, N) = 0)
      int ln = lane; asm volatile("" : "+v"(ln));
      const int lo = max(base[e], 0);
      const buf_t seg = buf_range(xs, lo, min(base[e] + L, nxu));
#pragma unroll
      for(int m = 0; m < P; m ++) S[ln + WAVE * m] = ld_range(seg, base[e] + ln + WAVE * m - lo);
#pragma unroll
      for(int m = 0; m <= H; m ++) {                                  // (lmax < N / 2: the lags lie in the lower registers)
        const int t = ln + WAVE * m;
        if(t <= lmax) R[t] = (e == 0 ? xr[m] : xi[m]) * (1.0f / (float)N);
      }
      __syncthreads();
      // E(0), float64: each lane its samples in rising order, then the butterfly over the lanes
      double e0 = 0.0;
      for(int t = lane; t < W; t += WAVE) e0 += (double)S[t] * (double)S[t];
      e0 = wave_sum_d(e0);
      // rule 3: the gate, against the utterance's mean square
      const double floor_u = nxu > 0 ? d.gate * uss[u] / (double)nxu : 0.0;
      float f0v = 0.0f;
      const bool gated = e0 == 0.0 || e0 / (double)W < floor_u;
      if(! gated) {
        // E(tau) - E(0) up to the lane's first lag: the lanes below hold q[j] = s[j+W]^2 - s[j]^2 of their chunks
        auto q = [&](int j) {
          // enters / leaves the window; S[L, N) is zero already, the guard only keeps j = lmax off S[N] when L == N
          const double in = j + W < L ? (double)S[j + W] : 0.0, out = (double)S[j];
          return in * in - out * out;
        };
        double tq = 0.0;
        for(int j = t0; j < t1; j ++) tq += q(j);
        const double e_base = e0 + wave_scan_excl_d(tq, lane);
        // the running sum of d up to the lane's first lag (d[0] is not part of it)
        double en = e_base, td = 0.0;
        for(int t = t0; t < t1; t ++) {
          if(t > 0) td += e0 + en - 2.0 * (double)R[t];
          en += q(t);
        }
        double cs = wave_scan_excl_d(td, lane);
        // rule 5, written over r
        en = e_base;
        for(int t = t0; t < t1; t ++) {
          const double dt = e0 + en - 2.0 * (double)R[t];
          float cm = 1.0f;
          if(t > 0) { cs += dt; cm = (float)(dt * (double)t / fmax(cs, 1e-12)); }
          en += q(t);
          R[t] = cm;
        }
        __syncthreads();
        if constexpr(CAND) {
          // rule T1.  Each lane owns the lags lmin + lane + 64 m: the local-minimum test per lag, the candidates' values
          // (else +inf) over the segment, which nobody reads any more, and the lane's lowest (value, lag)
          // (an opaque copy of the lane, as above: what is derived from it is formed here, not kept across the transforms)
          int ln = lane; asm volatile("" : "+v"(ln));
          float* C = S;
          // (F0_CB lags at a time, their reads issued together: one LDS latency per group, not per lag; a lag beyond the
          // row reads the last one again and is not looked at)
          float bv = INFINITY; int bt = 0x7fffffff;
          for(int tb = lmin + ln; tb < lmax; tb += F0_CB * WAVE) {
            float y0[F0_CB], y1[F0_CB], y2[F0_CB];
#pragma unroll
            for(int q = 0; q < F0_CB; q ++) {
              const int t = min(tb + q * WAVE, lmax - 1);
              y0[q] = R[t - 1]; y1[q] = R[t]; y2[q] = R[t + 1];
            }
#pragma unroll
            for(int q = 0; q < F0_CB; q ++) {
              const int t = tb + q * WAVE;
              const bool is = t < lmax && y1[q] < y0[q] && y1[q] <= y2[q] && y1[q] < c.threshold;
              if(t < lmax) C[t] = is ? y1[q] : INFINITY;
              if(is && y1[q] < bv) { bv = y1[q]; bt = t; }
            }
          }
          // seven rounds of a wave-wide arg-min over (value, lag) -- the least value, then the least lag among the lanes
          // that hold it; the lane that owned the winner strikes it out and looks through its lags again
          for(int k = 0; k < 7; k ++) {
            const float v = wave_min_f(bv);
            if(!(v < INFINITY)) break;                                // (the same on every lane)
            const int tv = wave_min_i(bv == v ? bt : 0x7fffffff);
            if(ln == 8 * e + k) { c_tau = tv; c_y0 = R[tv - 1]; c_y1 = v; c_y2 = R[tv + 1]; c_have = true; }
            if(((tv - lmin) & (WAVE - 1)) == ln) {
              C[tv] = INFINITY;
              bv = INFINITY; bt = 0x7fffffff;
              for(int tb = lmin + ln; tb < lmax; tb += F0_CB * WAVE) {
                float y[F0_CB];
#pragma unroll
                for(int q = 0; q < F0_CB; q ++) y[q] = C[min(tb + q * WAVE, lmax - 1)];
#pragma unroll
                for(int q = 0; q < F0_CB; q ++) { const int t = tb + q * WAVE; if(t < lmax && y[q] < bv) { bv = y[q]; bt = t; } }
              }
            }
          }
        } else {
          // rule 6: the first lag below the threshold, then down the slope to where it stops falling
          int tau = -1;
          for(int b0 = lmin; b0 < lmax && tau < 0; b0 += WAVE) {
            const int t = b0 + lane;
            const unsigned long long hit = __ballot(t < lmax && (double)R[t < lmax ? t : 0] < d.threshold);
            if(hit) tau = b0 + __ffsll((long long)hit) - 1;
          }
          if(tau >= 0) {
            for(int b0 = tau; ; b0 += WAVE) {
              const int t = b0 + lane;
              const bool falls = t + 1 < lmax && R[t + 1 < lmax ? t + 1 : 0] < R[t + 1 < lmax ? t : 0];
              const unsigned long long stop = __ballot(! falls);       // (t = lmax - 1 stops: the loop ends)
              if(stop) { tau = b0 + __ffsll((long long)stop) - 1; break; }
            }
            // rule 7 (lmin >= 2 and tau < lmax: both neighbours are lags of the row)
            const double y0 = (double)R[tau - 1], y1 = (double)R[tau], y2 = (double)R[tau + 1];
            const double den = y0 - 2.0 * y1 + y2;
            const double off = fabs(den) > 1e-12 ? 0.5 * (y0 - y2) / den : 0.0;
            f0v = (float)((double)d.fs / ((double)tau + off));
          }
        }
      }
      if(! CAND && lane == 0) raw[g] = f0v;
      if(cmndf) {
        float* row = cmndf + (size_t)g * (size_t)(lmax + 1);
        for(int t = lane; t <= lmax; t += WAVE) row[t] = gated ? 1.0f : R[t];
      }
      __syncthreads();                                                 // the next frame, or the next pair's transform, reuses the LDS
    }
    if constexpr(CAND) {
      // slot lane & 7 of the row of frame g0 + (lane >> 3): rule 7 of the lane's lag, and its logarithm
      float f0v = 0.0f, l2v = (lane & 7) == 7 ? c.L : 0.0f;
      if(c_have) {
        const double y0 = (double)c_y0, y1 = (double)c_y1, y2 = (double)c_y2;
        const double den = y0 - 2.0 * y1 + y2;
        const double off = fabs(den) > 1e-12 ? 0.5 * (y0 - y2) / den : 0.0;
        f0v = (float)((double)d.fs / ((double)c_tau + off));
        l2v = (float)log2((double)f0v);
      }
      if(lane < (two ? 16 : 8)) {
        float* row = c.plane + (size_t)(g0 + (lane >> 3)) * 24 + (lane & 7);
        row[0] = f0v; row[8] = c_y1; row[16] = l2v;
      }
    }
  }
}

// ---------------------------------------------------------------- median of five
// rule 8 over the raw values of each utterance; one thread per frame
__global__ __launch_bounds__(256) void k_f0_median(int nframes, const int* __restrict__ frm_utt,
  const int* __restrict__ frm_off, const int* __restrict__ nfrm, const float* __restrict__ raw, float* __restrict__ f0) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if(g >= nframes) return;
  const int u = frm_utt[g], i = g - frm_off[u], n = nfrm[u];
  float out = raw[g];
  if(i >= 2 && i < n - 2 && out != 0.0f) {
    float v[5]; int nz = 0;
#pragma unroll
    for(int k = 0; k < 5; k ++) {
      const float w = raw[g - 2 + k];
      v[k] = w != 0.0f ? w : INFINITY;                               // zeros sort behind the values
      nz += w != 0.0f;
    }
#pragma unroll
    for(int a = 1; a < 5; a ++)
#pragma unroll
      for(int b = a; b > 0; b --)
        if(v[b] < v[b - 1]) { const float t = v[b]; v[b] = v[b - 1]; v[b - 1] = t; }
    if(nz == 5) out = v[2];
    else if(nz == 4) out = __fmul_rn(__fadd_rn(v[1], v[2]), 0.5f);
    else if(nz <= 2) out = 0.0f;
  }
  f0[g] = out;
}

// ---------------------------------------------------------------- the path through the candidates
// Rules T2 - T5 of llsm_gpu_batch_track_f0, one wavefront per utterance.  Eight states (candidate slots 0 ... 6, and 7 =
// unvoiced) give 64 transitions: lane 8 j + a owns the one from state a of frame i - 1 to state j of frame i.  What does
// not depend on the running costs -- the local cost of j, the cost of the transition -- is formed for VIT_U frames at a
// time from rows loaded one such block ahead; the dependent chain of a frame is one addition, the (value, a) minimum over
// the eight lanes of a group, the local cost, the minimum over the groups, its subtraction, and the transposition that
// hands acc[a] to the lanes 8 j + a.  The back pointers, 3 bits per state, are one word per frame: lane i % 64 keeps the
// word of frame i and the wavefront stores 64 of them at a time.  The backtrack loads them 64 at a time as well and
// walks them with scalar reads of the lanes; lane k notes the state of frame base + k and fetches its F0 afterwards.
#define VIT_U 8
struct VitRows { float fj[VIT_U], f00[VIT_U], cj[VIT_U], lj[VIT_U], la[VIT_U]; };
// the rows of frames [base, base + VIT_U), as lane 8 j + a needs them; beyond the last frame: the last frame again
DEV void vit_load(VitRows& r, const float* __restrict__ rows, int base, int n, int j, int a) {
#pragma unroll
  for(int k = 0; k < VIT_U; k ++) {
    const float* row = rows + (size_t)min(base + k, n - 1) * 24;
    r.fj[k] = row[j]; r.f00[k] = row[0]; r.cj[k] = row[8 + j]; r.lj[k] = row[16 + j]; r.la[k] = row[16 + a];
  }
}

// the least of v over the eight groups, v being the same on the eight lanes of a group
DEV float vit_min_groups(float v) {
  v = fminf(v, dpp_f<DPP_ROR8>(v));
  return fminf(fminf(lane_f(v, 0), lane_f(v, 16)), fminf(lane_f(v, 32), lane_f(v, 48)));
}

__global__ __launch_bounds__(WAVE) void k_f0_viterbi(const int* __restrict__ frm_off, const int* __restrict__ nfrm,
  const float* __restrict__ plane, F0Track o, unsigned* __restrict__ bp, float* __restrict__ f0) {
  const int u = blockIdx.x, lane = threadIdx.x, j = lane >> 3, a = lane & 7;
  const int n = nfrm[u];
  if(n <= 0) return;
  const float* rows = plane + (size_t)frm_off[u] * 24;
  unsigned* bpu = bp + frm_off[u];
  float* out = f0 + frm_off[u];
  const float L = rows[23];
  float acc_a = 0.0f, acc_j = 0.0f, la_prev = 0.0f;                    // acc[a] of the frame before, acc[j] of this one
  unsigned word = 0;                                                    // the back pointers of frame (i & ~63) + lane
  VitRows cur, nxt;
  vit_load(cur, rows, 0, n, j, a);
  for(int b = 0; b < n; b += VIT_U) {
    vit_load(nxt, rows, b + VIT_U, n, j, a);
    float loc[VIT_U], tr[VIT_U];
#pragma unroll
    for(int k = 0; k < VIT_U; k ++) {
      // T2 (a slot is taken when its F0 is not zero)
      const float voiced = cur.fj[k] != 0.0f ? __fadd_rn(cur.cj[k], __fmul_rn(o.octave, __fsub_rn(L, cur.lj[k]))) : INFINITY;
      loc[k] = j < 7 ? voiced : (cur.f00[k] != 0.0f ? o.unvoiced : 0.0f);
      // T3
      const float lp = k == 0 ? la_prev : cur.la[k > 0 ? k - 1 : 0];
      tr[k] = j < 7 && a < 7 ? __fmul_rn(o.jump, fabsf(__fsub_rn(cur.lj[k], lp))) : (j == 7 && a == 7 ? 0.0f : o.sw);
      if(b + k == 0) tr[k] = 0.0f;                                     // acc_0 = loc_0
    }
    la_prev = cur.la[VIT_U - 1];
#pragma unroll
    for(int k = 0; k < VIT_U; k ++) {
      const int i = b + k;
      if(i >= n) break;
      // T4: the smallest a of the least acc[a] + tr(a, j), within the group of eight lanes
      float v = __fadd_rn(acc_a, tr[k]); int arg = a;
      auto take = [&](float ov, int oa) { if(ov < v || (ov == v && oa < arg)) { v = ov; arg = oa; } };
      take(dpp_f<DPP_XOR1>(v), dpp_i<DPP_XOR1>(arg));
      take(dpp_f<DPP_XOR2>(v), dpp_i<DPP_XOR2>(arg));
      // lane ^ 4 is 12 or 4 lanes round the row; both reads are made with every lane active, then one is chosen
      const float v_up = dpp_f<DPP_ROR12>(v), v_dn = dpp_f<DPP_ROR4>(v);
      const int a_up = dpp_i<DPP_ROR12>(arg), a_dn = dpp_i<DPP_ROR4>(arg);
      take(a < 4 ? v_up : v_dn, a < 4 ? a_up : a_dn);
      v = __fadd_rn(v, loc[k]);
      const float m = vit_min_groups(v);
      if(i > 0) v = __fsub_rn(v, m);
      acc_j = v;
      acc_a = __shfl(v, 8 * a, WAVE);
      // lane 3 s + t (below 24) contributes bit t of the back pointer of state s
      const int as = __shfl(arg, 8 * (lane / 3), WAVE);
      const unsigned w = (unsigned)__ballot(lane < 24 && ((as >> (lane % 3)) & 1));
      if((i & (WAVE - 1)) == lane) word = w;
      if(((i & (WAVE - 1)) == WAVE - 1 || i == n - 1) && lane <= (i & (WAVE - 1))) bpu[(i & ~(WAVE - 1)) + lane] = word;
    }
    cur = nxt;
  }
  // the path ends in the smallest state of least acc on the last frame
  const float m = vit_min_groups(acc_j);
  int s = __builtin_amdgcn_readfirstlane((__ffsll((long long)__ballot(acc_j == m)) - 1) >> 3);
  for(int base = (n - 1) & ~(WAVE - 1); base >= 0; base -= WAVE) {
    const int cnt = min(WAVE, n - base);
    const int w = lane < cnt ? (int)bpu[base + lane] : 0;             // (the lane's own stores: the same thread reads them)
    int st = 7;
#pragma unroll
    for(int k = WAVE - 1; k >= 0; k --) {
      if(k < cnt) {
        if(lane == k) st = s;
        s = ((unsigned)__builtin_amdgcn_readlane(w, k) >> (3 * s)) & 7;   // T4: state of frame base + k - 1
      }
    }
    if(lane < cnt) out[base + lane] = st < 7 ? rows[(size_t)(base + lane) * 24 + st] : 0.0f;   // T5
  }
}

// ---------------------------------------------------------------- launchers
int launch_f0_energy(LaunchCtx* P, const F0Dev& d, double* uss) {
  if(d.n_utt == 0) return 0;
  LAUNCH("k_f0_energy", k_f0_energy, dim3(d.n_utt), dim3(F0_EN_NT), 0, d.x, d.x_off, d.nx, uss);
  return 0;
}

int launch_f0_cmndf(LaunchCtx* P, const F0Dev& d, int logN, const double* uss, float* raw, float* cmndf, const F0Cand& c) {
  if(d.npairs == 0) return 0;
  // one instantiation per transform size wave_fft.h has, with and without the candidate search; -1: none for this size
  auto go = [&](auto ln, auto cand) {
    const size_t lds = sizeof(float2) * wf_lds_elems<ln>();
    // one-wavefront workgroups, each on a run of consecutive pairs: as many as stay resident, and 2048 at the least (a
    // floor, as for the other wavefront-FFT kernels: the runs are independent, so workgroups beyond the resident ones
    // -- LOGN 12 keeps 1024 -- simply follow them)
    const int grid = std::min(d.npairs, std::max(resident_blocks((const void*)k_f0_cmndf_wf<ln, cand>, WAVE, lds), 2048));
    LAUNCH(cand ? "k_f0_cmndf_wf_cand" : "k_f0_cmndf_wf", (k_f0_cmndf_wf<ln, cand>), dim3(grid), dim3(WAVE), lds, d, uss, raw,
      cmndf, c);
    return 0;
  };
  return pick_int<8, 9, 10, 11, 12>(logN, -1, [&](auto ln) {
    return c.plane ? go(ln, std::true_type{}) : go(ln, std::false_type{});
  });
}

int launch_f0_median(LaunchCtx* P, const F0Dev& d, const float* raw, float* f0) {
  if(d.nframes == 0) return 0;
  LAUNCH("k_f0_median", k_f0_median, dim3((d.nframes + 255) / 256), dim3(256), 0, d.nframes, d.frm_utt, d.frm_off, d.nfrm,
    raw, f0);
  return 0;
}

int launch_f0_viterbi(LaunchCtx* P, const F0Dev& d, const float* plane, const F0Track& t, unsigned* bp, float* f0) {
  if(d.n_utt == 0 || d.nframes == 0) return 0;
  LAUNCH("k_f0_viterbi", k_f0_viterbi, dim3(d.n_utt), dim3(WAVE), 0, d.frm_off, d.nfrm, plane, t, bp, f0);
  return 0;
}
