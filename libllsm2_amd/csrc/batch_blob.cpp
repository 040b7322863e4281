// batch_blob.cpp -- utterances of a device-resident batch as chunk blobs (wire.cpp's format, version 2), packed on the
// device: host side of blob_kernels.hip.  The other direction is llsm_gpu_batch_upload_blob(s) (l1.cpp).
//
//   llsm_blob_bytes                    bytes of a blob of a given shape (host only)
//   llsm_gpu_batch_blob_sizes          bytes of each utterance's blob as the batch stands now
//   llsm_gpu_batch_download_blobs      one destination per utterance
//   llsm_gpu_batch_download_blob_block all blobs back to back in one host block, at multiples of 16
//
// A call runs k_blob_widths over its utterances and fetches three ints per utterance; the host lays every blob out with
// wire_layout.h's layout() -- the one wire.cpp uses --, places the blobs at multiples of 16 in the batch's device staging
// area, in groups of at most 64 MiB, and uploads ONE table of headers and placements.  Per group k_blob_pack writes every
// byte of the area and one device-to-host copy takes it away: straight into a page-locked block, or into the batch's
// page-locked blob_stage (the one llsm_gpu_batch_upload_blobs uses) and from there to pageable destinations.  The batch's
// rows, min_f0 and f0_unknown are read, never written.  Rules and measurements: llsm_gpu.h, DESIGN.md section 19.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "batch.h"
#include "wire_layout.h"

using namespace llsm_wire;

namespace {
const size_t kStageBytes = (size_t)64 << 20;              // a group of blobs on the device and in blob_stage

size_t up16(size_t n) { return (n + 15) & ~(size_t)15; }

int refuse(const char* fn, const std::string& why) { llsm_set_error(std::string(fn) + ": " + why); return -1; }

int check_range(const char* fn, llsm_gpu_batch* b, int utt0, int n) {
  if(! b) return refuse(fn, "NULL batch");
  if(utt0 < 0 || n < 0 || utt0 > b -> lay.n_utt || n > b -> lay.n_utt - utt0)
    return refuse(fn, "utterances [" + std::to_string(utt0) + ", " + std::to_string((long long)utt0 + n) + ") are not within the batch's " +
      std::to_string(b -> lay.n_utt));
  return 0;
}

// The widths of utterances [utt0, utt0 + n) from the device, then each blob's header (entry k of the table in
// b -> blob_tab_h, chanfreq behind the entries).  Placements are not set yet.
int plan(const char* fn, llsm_gpu_batch* b, int utt0, int n) {
  hipSetDevice(b -> ctx -> device);
  hipStream_t st = b -> ctx -> stream;
  if(b -> blob_widths.alloc(3 * (size_t)n)) return -1;
  if(! b -> blob_widths_h.resize(3 * (size_t)n)) return -1;
  const int ncf = std::max(b -> lay.nchannel - 1, 0);       // LLSM_CONF_CHANFREQ as llsm_aoptions_toconf stores it
  if(! b -> blob_tab_h.resize((size_t)n * sizeof(BlobEntry) + (size_t)ncf * sizeof(float))) return -1;
  const int rc = launch_blob_widths(& b -> ctx -> lc, mod_rows(b), b -> d_frm_off.p + utt0, b -> d_nfrm.p + utt0, n, b -> blob_widths.p);
  if(rc) return refuse(fn, std::string("launch failed: ") + hipGetErrorString((hipError_t)rc));
  HIP_OK(hipMemcpyAsync(b -> blob_widths_h.data(), b -> blob_widths.p, 3 * (size_t)n * sizeof(int), hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  BlobEntry* tab = (BlobEntry*)b -> blob_tab_h.data();
  for(int k = 0; k < n; k ++) {
    const int* w = b -> blob_widths_h.data() + 3 * (size_t)k;
    Shape s;
    s.nfrm = b -> nfrm[utt0 + k]; s.maxnhar = std::max(w[0], w[1]); s.me = w[2];
    s.npsd = b -> lay.npsd; s.nch = b -> lay.nchannel; s.ncf = ncf; s.nspec = b -> l1_nspec;
    s.thop = b -> opt.thop; s.fnyq = b -> fnyq; s.lip = b -> opt.lip_radius; s.chanfreq = b -> chanfreq.data();
    std::memset(& tab[k], 0, sizeof(BlobEntry));
    fill_header(s, tab[k].h);
    tab[k].frm0 = b -> frm_off[utt0 + k];
  }
  if(ncf > 0) std::memcpy(tab + n, b -> chanfreq.data(), (size_t)ncf * sizeof(float));
  return 0;
}

// after plan(): no blob may exceed a group
int check_stage(const char* fn, llsm_gpu_batch* b, int utt0, int n) {
  const BlobEntry* tab = (const BlobEntry*)b -> blob_tab_h.data();
  for(int k = 0; k < n; k ++)
    if(up16(tab[k].h.total_bytes) > kStageBytes)
      return refuse(fn, "utterance " + std::to_string(utt0 + k) + " (" + std::to_string(tab[k].h.total_bytes) + " bytes) exceeds the staging area");
  return 0;
}

// Packs and copies.  block != NULL: blob k at block + the running multiple of 16; else blob k to dst[k].
int run(const char* fn, llsm_gpu_batch* b, int n, unsigned char* block, void* const* dst) {
  hipStream_t st = b -> ctx -> stream;
  BlobEntry* tab = (BlobEntry*)b -> blob_tab_h.data();
  // groups and placements
  std::vector<int> first; size_t widest = 0;
  for(int k = 0; k < n; ) {
    first.push_back(k);
    size_t at = 0;
    while(k < n && (at == 0 || at + up16(tab[k].h.total_bytes) <= kStageBytes)) { tab[k].base = at; at += up16(tab[k].h.total_bytes); k ++; }
    widest = std::max(widest, at);
  }
  first.push_back(n);
  bool pinned = false;
  if(block) {
    hipPointerAttribute_t at;
    pinned = hipPointerGetAttributes(& at, block) == hipSuccess && at.type == hipMemoryTypeHost;
    (void)hipGetLastError();                              // (ordinary memory is an error to the query, not to us)
  }
  if(! pinned && ! b -> blob_stage && hipHostMalloc(& b -> blob_stage, kStageBytes, hipHostMallocDefault) != hipSuccess) {
    b -> blob_stage = nullptr; (void)hipGetLastError();
    return refuse(fn, "page-locked staging allocation failed");
  }
  const size_t tab_bytes = b -> blob_tab_h.size();
  if(b -> blob_tab.alloc(tab_bytes) || b -> blob_dev.alloc(widest)) return -1;
  HIP_OK(hipMemcpyAsync(b -> blob_tab.p, tab, tab_bytes, hipMemcpyHostToDevice, st));
  const BlobEntry* dtab = (const BlobEntry*)b -> blob_tab.p;
  const float* dcf = (const float*)(dtab + n);
  size_t block_at = 0;
  for(size_t gi = 0; gi + 1 < first.size(); gi ++) {
    const int k0 = first[gi], k1 = first[gi + 1];
    int max_nfrm = 0; for(int k = k0; k < k1; k ++) max_nfrm = std::max(max_nfrm, tab[k].h.nfrm);
    const size_t bytes = tab[k1 - 1].base + up16(tab[k1 - 1].h.total_bytes);
    const int rc = launch_blob_pack(& b -> ctx -> lc, mod_rows(b), dtab + k0, dcf, k1 - k0, max_nfrm, b -> blob_dev.p);
    if(rc) return refuse(fn, std::string("launch failed: ") + hipGetErrorString((hipError_t)rc));
    if(pinned) HIP_OK(hipMemcpyAsync(block + block_at, b -> blob_dev.p, bytes, hipMemcpyDeviceToHost, st));   // the next group's kernel follows it on the stream
    else {
      HIP_OK(hipMemcpyAsync(b -> blob_stage, b -> blob_dev.p, bytes, hipMemcpyDeviceToHost, st));
      HIP_OK(hipStreamSynchronize(st));                   // blob_stage is reused by the next group
      if(block) std::memcpy(block + block_at, b -> blob_stage, bytes);
      else for(int k = k0; k < k1; k ++) std::memcpy(dst[k], (const char*)b -> blob_stage + tab[k].base, tab[k].h.total_bytes);
    }
    block_at += bytes;
  }
  HIP_OK(hipStreamSynchronize(st));
  return 0;
}
}  // namespace

extern "C" size_t llsm_blob_bytes(int nfrm, int maxnhar, int maxnhar_e, int npsd, int nchannel, int nchanfreq, int nspec) {
  if(nfrm < 0 || maxnhar < 0 || maxnhar_e < 0 || npsd < 0 || nchannel < 0 || nchanfreq < 0 || nspec < 0) {
    llsm_set_error("llsm_blob_bytes: negative dimension"); return 0;
  }
  Shape s;
  s.nfrm = nfrm; s.maxnhar = maxnhar; s.me = maxnhar_e; s.npsd = npsd; s.nch = nchannel; s.ncf = nchanfreq; s.nspec = nspec;
  return layout(s, nullptr);
}

extern "C" int llsm_gpu_batch_blob_sizes(llsm_gpu_batch* b, int utt0, int n, size_t* sizes) {
  const char* fn = "llsm_gpu_batch_blob_sizes";
  if(check_range(fn, b, utt0, n)) return -1;
  if(n == 0) return 0;
  if(! sizes) return refuse(fn, "NULL sizes");
  if(plan(fn, b, utt0, n)) return -1;
  const BlobEntry* tab = (const BlobEntry*)b -> blob_tab_h.data();
  for(int k = 0; k < n; k ++) sizes[k] = (size_t)tab[k].h.total_bytes;
  return 0;
}

extern "C" int llsm_gpu_batch_download_blobs(llsm_gpu_batch* b, int utt0, int n, void* const* dst, const size_t* capacity) {
  const char* fn = "llsm_gpu_batch_download_blobs";
  if(check_range(fn, b, utt0, n)) return -1;
  if(n == 0) return 0;
  if(! dst || ! capacity) return refuse(fn, "NULL destination table");
  for(int k = 0; k < n; k ++) {
    if(! dst[k]) return refuse(fn, "destination " + std::to_string(k) + " is NULL");
    if(((uintptr_t)dst[k] & 7u) != 0) return refuse(fn, "destination " + std::to_string(k) + " is not 8-byte aligned");
  }
  if(plan(fn, b, utt0, n)) return -1;
  const BlobEntry* tab = (const BlobEntry*)b -> blob_tab_h.data();
  for(int k = 0; k < n; k ++)
    if(capacity[k] < tab[k].h.total_bytes)
      return refuse(fn, "utterance " + std::to_string(utt0 + k) + " needs " + std::to_string(tab[k].h.total_bytes) + " bytes, capacity[" +
        std::to_string(k) + "] is " + std::to_string(capacity[k]));
  if(check_stage(fn, b, utt0, n)) return -1;
  return run(fn, b, n, nullptr, dst);
}

extern "C" int llsm_gpu_batch_download_blob_block(llsm_gpu_batch* b, int utt0, int n, void* block, size_t capacity, size_t* offsets) {
  const char* fn = "llsm_gpu_batch_download_blob_block";
  if(check_range(fn, b, utt0, n)) return -1;
  if(n == 0) { if(offsets) offsets[0] = 0; return 0; }
  if(! block || ! offsets) return refuse(fn, "NULL block or offsets");
  if(((uintptr_t)block & 7u) != 0) return refuse(fn, "block is not 8-byte aligned");
  if(plan(fn, b, utt0, n)) return -1;
  const BlobEntry* tab = (const BlobEntry*)b -> blob_tab_h.data();
  size_t need = 0;
  for(int k = 0; k < n; k ++) need += up16(tab[k].h.total_bytes);
  if(capacity < need)
    return refuse(fn, "utterances [" + std::to_string(utt0) + ", " + std::to_string(utt0 + n) + ") need " + std::to_string(need) +
      " bytes, the block holds " + std::to_string(capacity));
  if(check_stage(fn, b, utt0, n)) return -1;
  if(run(fn, b, n, (unsigned char*)block, nullptr)) return -1;
  size_t at = 0;
  for(int k = 0; k < n; k ++) { offsets[k] = at; at += up16(tab[k].h.total_bytes); }
  offsets[n] = at;
  return 0;
}
