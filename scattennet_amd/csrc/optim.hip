// Fused gradient-clip + Adam training update (include/scatten.h, "training update").
//
// Two launches replace clip_grad_norm_ + torch.optim.Adam.step() over every parameter tensor
// (opt.py:34-35 with the optimizer of optimizer.py:49-66).  The kernels are driven by tables
// in device memory (tensor table, chunk table, group table, state block) and stream over the
// chunk list in a fixed order, so nothing depends on the number of tensors and every result
// is bitwise reproducible from run to run: no float atomics, one partial per workgroup, and
// each element is summed by the same thread in the same order whether or not its tensor is
// 16-byte aligned (the unaligned path differs only in the width of its loads and stores).
#include "../../include/scatten.h"
#include "common.h"

namespace {

constexpr int OPT_THREADS = 256;
constexpr int OPT_DEFAULT_BLOCKS = 2048;  // 256 CUs x 8 workgroups of 256 threads

__host__ __device__ inline int optim_grid(int max_blocks, int nchunks) {
  const int cap = max_blocks > 0 ? max_blocks : OPT_DEFAULT_BLOCKS;
  const int g = nchunks < cap ? nchunks : cap;
  return g > 0 ? g : 1;
}

__device__ __forceinline__ bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// The table's pointers are generic; reading and writing through the GLOBAL address space
// gives global_load / global_store (a flat access also waits on the LDS counter).
typedef const __attribute__((address_space(1))) float cg_float;
typedef const __attribute__((address_space(1))) f32x4 cg_f32x4;
__device__ __forceinline__ float ld1(const float* p) { return *(cg_float*)p; }

__device__ __forceinline__ f32x4 load4(const float* p, bool vec) {
  if (vec) return *(cg_f32x4*)p;
  f32x4 v;
  v.x = ld1(p);
  v.y = ld1(p + 1);
  v.z = ld1(p + 2);
  v.w = ld1(p + 3);
  return v;
}

__device__ __forceinline__ void store4(float* p, f32x4 v, bool vec) {
  if (vec) {
    st4g(p, v);
  } else {
    st1g(p, v.x);
    st1g(p + 1, v.y);
    st1g(p + 2, v.z);
    st1g(p + 3, v.w);
  }
}

// Sum of v over the workgroup, the same bits in every thread: xor-butterfly inside each wave,
// then the four wave sums added in wave order.
__device__ __forceinline__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();  // red may still be read from an earlier call
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float s = red[0];
#pragma unroll
  for (int w = 1; w < OPT_THREADS / 64; ++w) s += red[w];
  return s;
}

// total gradient norm from the per-workgroup partials of sca_optim_grad_sqnorm: thread t adds
// partials t, t + 256, ... in order, then block_sum — every workgroup gets the same bits
__device__ __forceinline__ float total_norm(const float* partials, int npart, float* red) {
  float s = 0.0f;
  for (int i = threadIdx.x; i < npart; i += OPT_THREADS) s += ld1(partials + i);
  return sqrtf(block_sum(s, red));
}

// clip_grad_norm_'s coefficient: clamp(max_norm / (total + 1e-6), max = 1); a NaN stays a NaN
__device__ __forceinline__ float clip_coef(float total, float max_norm) {
  if (!(max_norm > 0.0f)) return 1.0f;
  const float c = max_norm / (total + 1e-6f);
  return c > 1.0f ? 1.0f : c;
}

__global__ __launch_bounds__(OPT_THREADS) void optim_grad_sqnorm_kernel(const sca_optim_tensor* __restrict__ tensors,
                                                                        const sca_optim_chunk* __restrict__ chunks,
                                                                        int nchunks, const float* __restrict__ loss,
                                                                        sca_optim_state* state,
                                                                        float* __restrict__ partials) {
  __shared__ float red[OPT_THREADS / 64];
  float acc = 0.0f;
  for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const sca_optim_chunk ch = chunks[c];
    const float* g = tensors[ch.tensor].g + ch.offset;
    const bool vec = aligned16(g);
    const int n4 = ch.len >> 2;
    for (int i = threadIdx.x; i < n4; i += OPT_THREADS) {
      const f32x4 v = load4(g + 4 * i, vec);
      acc += v.x * v.x;
      acc += v.y * v.y;
      acc += v.z * v.z;
      acc += v.w * v.w;
    }
    const int tail = 4 * n4 + threadIdx.x;
    if (tail < ch.len) acc += ld1(g + tail) * ld1(g + tail);
  }
  const float s = block_sum(acc, red);
  if (threadIdx.x == 0) {
    partials[blockIdx.x] = s;
    if (blockIdx.x == 0) {
      const int skipped = loss != nullptr && !isfinite(*loss);
      state->skipped = skipped;
      if (!skipped) state->step = state->step + 1;
    }
  }
}

struct StepConsts {
  float coef, wd, w1, b2, w2, eps, step_size, bc2_sqrt;
};

__global__ __launch_bounds__(OPT_THREADS) void optim_adam_step_kernel(const sca_optim_tensor* __restrict__ tensors,
                                                                      const sca_optim_chunk* __restrict__ chunks,
                                                                      int nchunks,
                                                                      const sca_optim_group* __restrict__ groups,
                                                                      int npart, float max_norm,
                                                                      sca_optim_state* state,
                                                                      const float* __restrict__ partials) {
  __shared__ float red[OPT_THREADS / 64];
  __shared__ float hyper[7];
  const float total = total_norm(partials, npart, red);
  const float coef = clip_coef(total, max_norm);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    state->grad_norm = total;
    state->clip_coef = coef;
  }
  if (state->skipped) return;
  const int step = state->step;
  for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const sca_optim_chunk ch = chunks[c];
    const sca_optim_tensor t = tensors[ch.tensor];
    __syncthreads();  // the previous chunk's readers of hyper[] are done
    if (threadIdx.x == 0) {
      // torch.optim.Adam's scalars: python doubles, rounded to fp32 where they meet a tensor
      const sca_optim_group h = groups[t.group];
      const int ts = step - t.t0 > 1 ? step - t.t0 : 1;  // a tensor's own step count (>= 1)
      const double bc1 = 1.0 - pow(h.beta1, (double)ts);
      const double bc2 = 1.0 - pow(h.beta2, (double)ts);
      hyper[0] = (float)h.weight_decay;
      hyper[1] = (float)(1.0 - h.beta1);
      hyper[2] = (float)h.beta2;
      hyper[3] = (float)(1.0 - h.beta2);
      hyper[4] = (float)h.eps;
      hyper[5] = (float)(h.lr / bc1);
      hyper[6] = (float)sqrt(bc2);
    }
    __syncthreads();
    StepConsts k;
    k.coef = coef;
    k.wd = hyper[0];
    k.w1 = hyper[1];
    k.b2 = hyper[2];
    k.w2 = hyper[3];
    k.eps = hyper[4];
    k.step_size = hyper[5];
    k.bc2_sqrt = hyper[6];
    float* p = t.p + ch.offset;
    const float* g = t.g + ch.offset;
    float* m = t.exp_avg + ch.offset;
    float* v = t.exp_avg_sq + ch.offset;
    float* vmax = t.max_exp_avg_sq ? t.max_exp_avg_sq + ch.offset : nullptr;
    const bool vec = aligned16(p) && aligned16(g) && aligned16(m) && aligned16(v) && aligned16(vmax);

    auto update = [&](float& pe, float ge, float& me, float& ve, float& xe) {
      float gp = k.coef * ge;
      gp = gp + k.wd * pe;
      me = me + k.w1 * (gp - me);
      ve = ve * k.b2;
      ve = ve + k.w2 * gp * gp;
      float vh = ve;
      if (vmax) {
        xe = fmaxf(xe, ve);
        vh = xe;
      }
      const float denom = sqrtf(vh) / k.bc2_sqrt + k.eps;
      pe = pe - k.step_size * (me / denom);
    };

    const int n4 = ch.len >> 2;
    for (int i = threadIdx.x; i < n4; i += OPT_THREADS) {
      f32x4 p4 = load4(p + 4 * i, vec);
      const f32x4 g4 = load4(g + 4 * i, vec);
      f32x4 m4 = load4(m + 4 * i, vec);
      f32x4 v4 = load4(v + 4 * i, vec);
      f32x4 x4 = {0.0f, 0.0f, 0.0f, 0.0f};
      if (vmax) x4 = load4(vmax + 4 * i, vec);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float pe = p4[e], me = m4[e], ve = v4[e], xe = x4[e];
        update(pe, g4[e], me, ve, xe);
        p4[e] = pe;
        m4[e] = me;
        v4[e] = ve;
        x4[e] = xe;
      }
      store4(p + 4 * i, p4, vec);
      store4(m + 4 * i, m4, vec);
      store4(v + 4 * i, v4, vec);
      if (vmax) store4(vmax + 4 * i, x4, vec);
    }
    const int tail = 4 * n4 + threadIdx.x;
    if (tail < ch.len) {
      float pe = ld1(p + tail), me = ld1(m + tail), ve = ld1(v + tail), xe = vmax ? ld1(vmax + tail) : 0.0f;
      update(pe, ld1(g + tail), me, ve, xe);
      st1g(p + tail, pe);
      st1g(m + tail, me);
      st1g(v + tail, ve);
      if (vmax) st1g(vmax + tail, xe);
    }
  }
}

__global__ __launch_bounds__(OPT_THREADS) void optim_scale_grads_kernel(const sca_optim_tensor* __restrict__ tensors,
                                                                        const sca_optim_chunk* __restrict__ chunks,
                                                                        int nchunks, int npart, float max_norm,
                                                                        sca_optim_state* state,
                                                                        const float* __restrict__ partials) {
  __shared__ float red[OPT_THREADS / 64];
  const float total = total_norm(partials, npart, red);
  const float coef = clip_coef(total, max_norm);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    state->grad_norm = total;
    state->clip_coef = coef;
  }
  if (coef == 1.0f) return;  // g * 1 is g
  for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const sca_optim_chunk ch = chunks[c];
    float* g = tensors[ch.tensor].g + ch.offset;
    const bool vec = aligned16(g);
    const int n4 = ch.len >> 2;
    for (int i = threadIdx.x; i < n4; i += OPT_THREADS) {
      f32x4 v = load4(g + 4 * i, vec);
      v.x *= coef;
      v.y *= coef;
      v.z *= coef;
      v.w *= coef;
      store4(g + 4 * i, v, vec);
    }
    const int tail = 4 * n4 + threadIdx.x;
    if (tail < ch.len) st1g(g + tail, ld1(g + tail) * coef);
  }
}

bool bad_tables(const void* tensors, const void* chunks, int nchunks, const void* state, const void* partials) {
  return nchunks < 0 || !state || !partials || (nchunks > 0 && (!tensors || !chunks));
}

}  // namespace

extern "C" int sca_optim_blocks(int max_blocks, int nchunks) { return optim_grid(max_blocks, nchunks); }

extern "C" int sca_optim_grad_sqnorm(const sca_optim_tensor* tensors, const sca_optim_chunk* chunks, int nchunks,
                                     int max_blocks, const float* loss, sca_optim_state* state, float* partials,
                                     void* stream) {
  if (bad_tables(tensors, chunks, nchunks, state, partials) || max_blocks < 0) {
    sca_set_error("sca_optim_grad_sqnorm: bad arguments");
    return SCA_ERR_ARG;
  }
  hipLaunchKernelGGL(optim_grad_sqnorm_kernel, dim3(optim_grid(max_blocks, nchunks)), dim3(OPT_THREADS), 0,
                     (hipStream_t)stream, tensors, chunks, nchunks, loss, state, partials);
  return sca_launch_status("sca_optim_grad_sqnorm");
}

extern "C" int sca_optim_adam_step(const sca_optim_tensor* tensors, const sca_optim_chunk* chunks, int nchunks,
                                   const sca_optim_group* groups, int max_blocks, float max_norm,
                                   sca_optim_state* state, const float* partials, void* stream) {
  if (bad_tables(tensors, chunks, nchunks, state, partials) || max_blocks < 0 || (nchunks > 0 && !groups)) {
    sca_set_error("sca_optim_adam_step: bad arguments");
    return SCA_ERR_ARG;
  }
  const int grid = optim_grid(max_blocks, nchunks);  // also the number of partials of pass 1
  hipLaunchKernelGGL(optim_adam_step_kernel, dim3(grid), dim3(OPT_THREADS), 0, (hipStream_t)stream, tensors, chunks,
                     nchunks, groups, grid, max_norm, state, partials);
  return sca_launch_status("sca_optim_adam_step");
}

extern "C" int sca_optim_scale_grads(const sca_optim_tensor* tensors, const sca_optim_chunk* chunks, int nchunks,
                                     int max_blocks, float max_norm, sca_optim_state* state, const float* partials,
                                     void* stream) {
  if (bad_tables(tensors, chunks, nchunks, state, partials) || max_blocks < 0) {
    sca_set_error("sca_optim_scale_grads: bad arguments");
    return SCA_ERR_ARG;
  }
  const int grid = optim_grid(max_blocks, nchunks);
  hipLaunchKernelGGL(optim_scale_grads_kernel, dim3(grid), dim3(OPT_THREADS), 0, (hipStream_t)stream, tensors, chunks,
                     nchunks, grid, max_norm, state, partials);
  return sca_launch_status("sca_optim_scale_grads");
}

extern "C" int sca_optim_upload(void* dst, const void* src, long bytes, void* stream) {
  if (bytes < 0 || (bytes > 0 && (!dst || !src))) {
    sca_set_error("sca_optim_upload: bad arguments");
    return SCA_ERR_ARG;
  }
  if (bytes == 0) return SCA_OK;
  if (hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyHostToDevice, (hipStream_t)stream) != hipSuccess) {
    (void)hipGetLastError();
    sca_set_error("sca_optim_upload: hipMemcpyAsync failed");
    return SCA_ERR_LAUNCH;
  }
  return SCA_OK;
}
