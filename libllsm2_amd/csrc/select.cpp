// select.cpp -- unit selection on the device: host side of select_kernels.hip.
//
//   llsm_gpu_select_default_options  the defaults of llsm_gpu.h
//   llsm_gpu_select_check            host only: every refusal that needs no batch beyond the orders of its coder
//   llsm_gpu_batch_select            LLSM_GPU_CODE of a target batch and of a bank -> for every target frame the bank frame
//                                    that renders it, as splice takes it, and the path cost per utterance (rules S1 - S5:
//                                    llsm_gpu.h): the eight nearest bank frames of every target frame
//                                    (k_select_knn per bank segment, k_select_merge), the join costs between the candidates
//                                    of neighbouring frames (k_select_join), one path per utterance (k_select_path), one
//                                    copy back
//
// Every check runs before anything is allocated, copied or launched.  The scratch lives on batch t, grow-only.  The
// utterance tables of both batches (frame offsets, frame counts, frame -> utterance) are on the device since the batches
// were made, so the call uploads nothing.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "batch.h"

namespace {
const char* kSelect = "llsm_gpu_batch_select";
const long long kMaxBank = 1ll << 24;             // plane 7 keeps frame indices as floats

int refuse(const std::string& why) { llsm_set_error(std::string(kSelect) + ": " + why); return -1; }

// the options checked against a coder of these orders, count resolved; -1 with the error set
int check(llsm_gpu_select_options* o, int order_spec, int order_bap) {
  if(order_spec < 1 || order_bap < 1) return refuse("the coder is not enabled");
  const int dim = order_spec + order_bap + 3;
  if(o -> count <= 0) o -> count = order_spec;
  if(o -> first < 0 || o -> first >= dim || o -> count > dim - o -> first)
    return refuse("columns [" + std::to_string(o -> first) + ", " + std::to_string((long long)o -> first + o -> count) +
      ") lie outside [0, " + std::to_string(dim) + ")");
  if(std::isnan(o -> voicing_cost) || std::isnan(o -> join_cost)) return refuse("a cost is NaN");
  if(std::isnan(o -> join_weight)) return refuse("join_weight is NaN");
  if(std::isinf(o -> voicing_cost) || std::isinf(o -> join_cost)) return refuse("a cost is infinite");
  if(std::isinf(o -> join_weight)) return refuse("join_weight is infinite");
  if(o -> voicing_cost < 0) return refuse("voicing_cost < 0");
  if(o -> join_cost < 0) return refuse("join_cost < 0");
  if(o -> join_weight < 0) return refuse("join_weight < 0");
  if(o -> skip_own_utterance != 0 && o -> skip_own_utterance != 1)
    return refuse("skip_own_utterance is " + std::to_string(o -> skip_own_utterance) + ", not 0 or 1");
  return 0;
}
}  // namespace

extern "C" void llsm_gpu_select_default_options(llsm_gpu_select_options* dst) {
  if(! dst) return;
  dst -> first = 3; dst -> count = 0; dst -> voicing_cost = 0; dst -> join_cost = 0; dst -> join_weight = 1;
  dst -> skip_own_utterance = 0;
}

extern "C" int llsm_gpu_select_check(const llsm_gpu_select_options* opt, int order_spec, int order_bap) {
  llsm_gpu_select_options o;
  if(opt) o = *opt; else llsm_gpu_select_default_options(& o);
  return check(& o, order_spec, order_bap);
}

extern "C" int llsm_gpu_batch_select(llsm_gpu_batch* t, const llsm_gpu_batch* bank, const llsm_gpu_select_options* opt,
  int* utt, FP_TYPE* pos, FP_TYPE* cost) {
  if(! t || ! bank) return refuse("NULL batch");
  if(t -> ctx != bank -> ctx) return refuse("the batches belong to different contexts");
  if(t -> coder_os == 0 || bank -> coder_os == 0) return refuse("the coder is not enabled on both batches");
  if(t -> coder_os + t -> coder_ob != bank -> coder_os + bank -> coder_ob)
    return refuse("the coder dimensions differ: " + std::to_string(t -> coder_os + t -> coder_ob + 3) + " and " +
      std::to_string(bank -> coder_os + bank -> coder_ob + 3));
  llsm_gpu_select_options o;
  if(opt) o = *opt; else llsm_gpu_select_default_options(& o);
  if(check(& o, t -> coder_os, t -> coder_ob)) return -1;
  if(o.skip_own_utterance && t != bank) return refuse("skip_own_utterance needs t == bank");
  const long long nt = t -> lay.total_frames, nb = bank -> lay.total_frames;
  const int n_utt = t -> lay.n_utt;
  if(nt == 0) {                                                     // nothing to select: every cost is 0
    if(cost) std::fill(cost, cost + n_utt, (FP_TYPE)0);
    return 0;
  }
  if(! utt) return refuse("NULL utt");
  if(! pos) return refuse("NULL pos");
  if(nb == 0) return refuse("the bank has no frames");
  if(nb > kMaxBank) return refuse("the bank holds " + std::to_string(nb) + " frames, more than 2^24 = " + std::to_string(kMaxBank));
  if(o.skip_own_utterance)
    for(int u = 0; u < n_utt; u ++)
      if(t -> nfrm[u] > 0 && nb - t -> nfrm[u] <= 0)
        return refuse("skip_own_utterance leaves utterance " + std::to_string(u) + " without a bank frame");
  // accepted: from here on t's scratch changes
  hipSetDevice(t -> ctx -> device);
  SelectDev d;
  d.code_t = (const float*)t -> arr[LLSM_GPU_CODE]; d.code_b = (const float*)bank -> arr[LLSM_GPU_CODE];
  d.dim = t -> coder_os + t -> coder_ob + 3; d.first = o.first; d.count = o.count;
  d.voicing_cost = o.voicing_cost; d.join_cost = o.join_cost; d.join_weight = o.join_weight; d.skip_own = o.skip_own_utterance;
  d.nt = (int)nt; d.nb = (int)nb; d.n_utt = n_utt;
  d.t_frm_off = t -> d_frm_off.p; d.t_nfrm = t -> d_nfrm.p; d.t_frm_utt = t -> d_frm_utt.p;
  d.b_frm_off = bank -> d_frm_off.p; d.b_nfrm = bank -> d_nfrm.p; d.b_frm_utt = bank -> d_frm_utt.p;
  d.seg_len = select_seg_len(d.nb); d.n_seg = select_segments(d.nb);
  const size_t n_out = 2 * (size_t)nt + (size_t)n_utt;
  t -> sel_frames = 0;                    // from here on the planes of an earlier call may be gone (a buffer that grows is
                                          // freed first): they are readable again once this call has succeeded
  if((d.n_seg > 1 && t -> sel_lists.alloc((size_t)d.n_seg * nt * 16)) || t -> sel_p7.alloc((size_t)nt * 16) ||
     t -> sel_p8.alloc((size_t)nt * 64) || t -> sel_bp.alloc((size_t)nt) || t -> sel_out.alloc(n_out)) return -1;
  LaunchCtx* P = & t -> ctx -> lc;
  int rc = launch_select_knn(P, d, d.n_seg > 1 ? t -> sel_lists.p : t -> sel_p7.p);
  if(! rc && d.n_seg > 1) rc = launch_select_merge(P, d, t -> sel_lists.p, t -> sel_p7.p);
  if(! rc) rc = launch_select_join(P, d, t -> sel_p7.p, t -> sel_p8.p);
  if(! rc) rc = launch_select_path(P, d, t -> sel_p7.p, t -> sel_p8.p, t -> sel_bp.p, t -> sel_out.p);
  if(rc) return refuse(std::string("launch failed: ") + hipGetErrorString((hipError_t)rc));
  // into memory of our own first: a failed copy leaves the three arrays untouched
  std::vector<int> host(n_out);
  HIP_OK(hipMemcpyAsync(host.data(), t -> sel_out.p, n_out * sizeof(int), hipMemcpyDeviceToHost, P -> stream));
  HIP_OK(hipStreamSynchronize(P -> stream));
  std::copy(host.begin(), host.begin() + nt, utt);
  const float* fh = (const float*)host.data();
  std::copy(fh + nt, fh + 2 * nt, pos);
  if(cost) std::copy(fh + 2 * nt, fh + n_out, cost);
  t -> sel_frames = nt;
  return 0;
}
