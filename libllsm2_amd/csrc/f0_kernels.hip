// f0_kernels.hip -- F0 estimation of a batch's waveforms (llsm_gpu_batch_estimate_f0; rules: llsm_gpu.h, DESIGN.md
// section 21; host side: f0.cpp).  Three kernels:
//
//   k_f0_energy      sum of squares of every utterance, float64, in an order fixed by the utterance's length
//   k_f0_cmndf_wf    one wavefront per frame pair on the register-resident wavefront FFT (wave_fft.h): the YIN difference
//                    function through a cross-correlation, the cumulative-mean-normalised difference (CMNDF), the lag
//                    search and the parabolic fit -> one raw F0 per frame
//   k_f0_median      the median-of-5 pass over the raw row of each utterance
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

template <int LOGN>
__global__ __launch_bounds__(WAVE, (LOGN >= 12 ? 1 : 2)) void k_f0_cmndf_wf(F0Dev d, const double* __restrict__ uss,
  float* __restrict__ raw, float* __restrict__ cmndf) {
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
      if(lane == 0) raw[g] = f0v;
      if(cmndf) {
        float* row = cmndf + (size_t)g * (size_t)(lmax + 1);
        for(int t = lane; t <= lmax; t += WAVE) row[t] = gated ? 1.0f : R[t];
      }
      __syncthreads();                                                 // the next frame, or the next pair's transform, reuses the LDS
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

// ---------------------------------------------------------------- launchers
int launch_f0_energy(LaunchCtx* P, const F0Dev& d, double* uss) {
  if(d.n_utt == 0) return 0;
  LAUNCH("k_f0_energy", k_f0_energy, dim3(d.n_utt), dim3(F0_EN_NT), 0, d.x, d.x_off, d.nx, uss);
  return 0;
}

int launch_f0_cmndf(LaunchCtx* P, const F0Dev& d, int logN, const double* uss, float* raw, float* cmndf) {
  if(d.npairs == 0) return 0;
  // one instantiation per transform size wave_fft.h has; -1: none for this size
  return pick_int<8, 9, 10, 11, 12>(logN, -1, [&](auto ln) {
    const size_t lds = sizeof(float2) * wf_lds_elems<ln>();
    // one-wavefront workgroups, each on a run of consecutive pairs: as many as stay resident, and 2048 at the least (a
    // floor, as for the other wavefront-FFT kernels: the runs are independent, so workgroups beyond the resident ones
    // -- LOGN 12 keeps 1024 -- simply follow them)
    const int grid = std::min(d.npairs, std::max(resident_blocks((const void*)k_f0_cmndf_wf<ln>, WAVE, lds), 2048));
    LAUNCH("k_f0_cmndf_wf", (k_f0_cmndf_wf<ln>), dim3(grid), dim3(WAVE), lds, d, uss, raw, cmndf);
    return 0;
  });
}

int launch_f0_median(LaunchCtx* P, const F0Dev& d, const float* raw, float* f0) {
  if(d.nframes == 0) return 0;
  LAUNCH("k_f0_median", k_f0_median, dim3((d.nframes + 255) / 256), dim3(256), 0, d.nframes, d.frm_utt, d.frm_off, d.nfrm,
    raw, f0);
  return 0;
}
