// Device-side finite guard of the training step (include/scatten.h, "finite guard").
//
// MSCA_Net.forward tests about thirty tensors with isnan().any() / isinf().any()
// (model/__init__.py:130-235), each a reduction launch plus a host read that drains the
// queue.  sca_finite_scan reads all of them in ONE launch and leaves one 32-bit flag word per
// tensor (bit 0: a NaN, bit 1: a +-Inf); sca_step_report gathers the flag words and the loss
// terms into one contiguous buffer — the only thing the host reads, once per step, or never
// under graph capture — and writes the `guard` scalar that FusedAdam.step(loss=...) tests on
// the device.
//
// The tensors' (pointer, numel) pairs travel by value in the kernel arguments: no device
// table, nothing to upload, safe under stream capture.  Elements are classified from their
// exponent and mantissa bits with integer compares, so no floating-point flag or folding
// rule can change the answer, and the answer does not depend on the width of the loads.
#include "../../include/scatten.h"
#include "common.h"

namespace {

constexpr int GUARD_THREADS = 256;
constexpr int GUARD_MAX_BLOCKS = 2048;  // 256 CUs x 8 workgroups of 256 threads
constexpr int GUARD_CHUNK = SCA_GUARD_CHUNK;
static_assert(GUARD_CHUNK % (4 * GUARD_THREADS) == 0, "a chunk is whole rounds of 16-byte loads");

struct ScanArgs {
  const float* ptr[SCA_GUARD_MAX_TENSORS];
  long numel[SCA_GUARD_MAX_TENSORS];
  int first_chunk[SCA_GUARD_MAX_TENSORS + 1];  // chunks never span two tensors
  int ntensors;
};

typedef const __attribute__((address_space(1))) uint32_t cg_u32;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(1))) u32x4 cg_u32x4;

// bit 0: NaN (exponent all ones, mantissa non-zero); bit 1: +-Inf (mantissa zero)
__device__ __forceinline__ uint32_t classify(uint32_t u) {
  const uint32_t a = u & 0x7fffffffu;
  return (a > 0x7f800000u ? 1u : 0u) | (a == 0x7f800000u ? 2u : 0u);
}

__global__ __launch_bounds__(GUARD_THREADS) void finite_scan_kernel(ScanArgs a, uint32_t* __restrict__ flags) {
  __shared__ uint32_t found[SCA_GUARD_MAX_TENSORS];
  if (threadIdx.x < SCA_GUARD_MAX_TENSORS) found[threadIdx.x] = 0;
  __syncthreads();
  const int nchunks = a.first_chunk[a.ntensors];
  int t = 0;
  for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
    while (c >= a.first_chunk[t + 1]) ++t;  // uniform: chunks are in tensor order
    const long off = (long)(c - a.first_chunk[t]) * GUARD_CHUNK;
    const long left = a.numel[t] - off;
    const int len = left < GUARD_CHUNK ? (int)left : GUARD_CHUNK;
    const uint32_t* p = reinterpret_cast<const uint32_t*>(a.ptr[t]) + off;
    // elements before the first 16-byte boundary (0..3), then 16-byte loads, then the rest
    int head = (int)((16 - (reinterpret_cast<uintptr_t>(p) & 15)) & 15) >> 2;
    if (head > len) head = len;
    const int n4 = (len - head) >> 2;
    const int tail = head + 4 * n4;
    uint32_t bits = 0;
    if ((int)threadIdx.x < head) bits |= classify(*(cg_u32*)(p + threadIdx.x));
    for (int i = threadIdx.x; i < n4; i += GUARD_THREADS) {
      const u32x4 v = *(cg_u32x4*)(p + head + 4 * i);
      bits |= classify(v.x) | classify(v.y) | classify(v.z) | classify(v.w);
    }
    if (tail + (int)threadIdx.x < len) bits |= classify(*(cg_u32*)(p + tail + threadIdx.x));
    const uint32_t wave = (__any(bits & 1u) ? 1u : 0u) | (__any(bits & 2u) ? 2u : 0u);
    if (wave && (threadIdx.x & 63) == 0) atomicOr(&found[t], wave);  // LDS
  }
  __syncthreads();
  // at most one global atomic per tensor and workgroup, none on a clean step
  if ((int)threadIdx.x < a.ntensors && found[threadIdx.x]) atomicOr(flags + threadIdx.x, found[threadIdx.x]);
}

__global__ __launch_bounds__(64) void flags_clear_kernel(uint32_t* __restrict__ flags, int n) {
  if ((int)threadIdx.x < n) flags[threadIdx.x] = 0u;  // n <= SCA_GUARD_MAX_TENSORS
}

struct ReportArgs {
  const float* distill[SCA_REPORT_MAX_DISTILL];
  int ndistill;
};

// One wave.  report words: [0, nflags) flag words, then fp32: alignment_loss, fuse_coord_loss,
// the distillation terms, total_loss, guard.
__global__ __launch_bounds__(64) void step_report_kernel(const uint32_t* __restrict__ flags, int nflags,
                                                         const float* __restrict__ alignment_loss,
                                                         const float* __restrict__ fuse_coord_loss, ReportArgs d,
                                                         float* __restrict__ total_loss, uint32_t* __restrict__ report) {
  uint32_t any = 0;
  for (int i = threadIdx.x; i < nflags; i += 64) {
    const uint32_t f = flags ? flags[i] : 0u;
    report[i] = f;
    any |= f;
  }
  const bool flagged = __any(any != 0);
  if (threadIdx.x == 0) {
    float* out = reinterpret_cast<float*>(report + nflags);
    // model/__init__.py:207,237: total = fuse_coord_loss, then += each term in cfg order
    float total = *fuse_coord_loss;
    out[0] = alignment_loss ? *alignment_loss : 0.0f;
    out[1] = total;
    for (int k = 0; k < d.ndistill; ++k) {
      const float v = *d.distill[k];
      out[2 + k] = v;
      total += v;
    }
    out[2 + d.ndistill] = total;
    out[3 + d.ndistill] = flagged ? __uint_as_float(0x7fc00000u) : total;
    if (total_loss) *total_loss = total;
  }
}

}  // namespace

extern "C" int sca_finite_scan(int ntensors, const float* const* ptrs, const long* numels, unsigned* flags,
                               void* stream) {
  if (ntensors < 0 || ntensors > SCA_GUARD_MAX_TENSORS || (ntensors > 0 && (!ptrs || !numels || !flags))) {
    sca_set_error("sca_finite_scan: 0..16 tensors, with ptrs, numels and flags");
    return SCA_ERR_ARG;
  }
  if (ntensors == 0) return SCA_OK;
  ScanArgs a = {};
  a.ntensors = ntensors;
  long chunks = 0;
  for (int t = 0; t < ntensors; ++t) {
    if (numels[t] < 0 || (numels[t] > 0 && !ptrs[t]) || (reinterpret_cast<uintptr_t>(ptrs[t]) & 3)) {
      sca_set_error("sca_finite_scan: a tensor has a negative size, a null pointer or is not 4-byte aligned");
      return SCA_ERR_ARG;
    }
    a.ptr[t] = ptrs[t];
    a.numel[t] = numels[t];
    a.first_chunk[t] = (int)chunks;
    chunks += (numels[t] + GUARD_CHUNK - 1) / GUARD_CHUNK;
    if (chunks > 0x7fffffffL) {
      sca_set_error("sca_finite_scan: too many elements for one launch");
      return SCA_ERR_ARG;
    }
  }
  for (int t = ntensors; t <= SCA_GUARD_MAX_TENSORS; ++t) a.first_chunk[t] = (int)chunks;
  // the flag words are cleared on the stream, then OR-ed into.  A kernel, not hipMemsetAsync: a
  // memset node of a replayed graph was seen to fill the words with a stale 16-byte pattern
  // once the host had made enough pageable copies in between (evaluation step)
  hipLaunchKernelGGL(flags_clear_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, flags, ntensors);
  if (chunks == 0) {
    return sca_launch_status("sca_finite_scan");
  }
  const int grid = chunks < GUARD_MAX_BLOCKS ? (int)chunks : GUARD_MAX_BLOCKS;
  hipLaunchKernelGGL(finite_scan_kernel, dim3(grid), dim3(GUARD_THREADS), 0, (hipStream_t)stream, a, flags);
  return sca_launch_status("sca_finite_scan");
}

extern "C" int sca_step_report(const unsigned* flags, int nflags, const float* alignment_loss,
                               const float* fuse_coord_loss, int ndistill, const float* const* distill,
                               float* total_loss, void* report, void* stream) {
  if (nflags < 0 || nflags > SCA_REPORT_MAX_FLAGS || ndistill < 0 || ndistill > SCA_REPORT_MAX_DISTILL ||
      !fuse_coord_loss || !report || (ndistill > 0 && !distill)) {
    sca_set_error("sca_step_report: bad arguments");
    return SCA_ERR_ARG;
  }
  ReportArgs d = {};
  d.ndistill = ndistill;
  for (int k = 0; k < ndistill; ++k) {
    if (!distill[k]) { sca_set_error("sca_step_report: null distillation term"); return SCA_ERR_ARG; }
    d.distill[k] = distill[k];
  }
  hipLaunchKernelGGL(step_report_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, flags, nflags, alignment_loss,
                     fuse_coord_loss, d, total_loss, static_cast<uint32_t*>(report));
  return sca_launch_status("sca_step_report");
}
