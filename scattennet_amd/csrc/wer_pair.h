// The project's WER alignment of one (reference, hypothesis) pair (include/scatten.h,
// sca_wer_counts), shared by the WER kernel, the evaluation step, MBR selection (decode.hip)
// and the MWER loss (mwer.hip): one device function, so that all of them count errors alike.
#pragma once
#include "common.h"
#include "../../include/scatten.h"

namespace {

constexpr int WER_LD = SCA_WER_MAX_LEN + 3;  // odd dword stride along an anti-diagonal
constexpr int WER_DEL = 3, WER_INS = 3, WER_SUB = 4;

// One workgroup (128 threads) per (reference, hypothesis) pair; thread i owns matrix row i + 1
// and the matrix is filled one anti-diagonal per barrier.  Thread 0 walks the alignment back
// and writes out[0..4) = (num_del, num_ins, num_sub, num_ref); the other threads' `out` is
// not touched.  R <= SCA_WER_MAX_LEN tokens at r, H <= SCA_WER_MAX_LEN at h (both clamped by
// the caller).  Ends with the hypothesis still in h_s for thread-parallel readers.
__device__ __forceinline__ void wer_pair(const int* __restrict__ r, int R, const int* __restrict__ h, int H,
                                         int* __restrict__ out) {
  __shared__ unsigned short dm[(SCA_WER_MAX_LEN + 1) * WER_LD];
  __shared__ int r_s[SCA_WER_MAX_LEN], h_s[SCA_WER_MAX_LEN];
  const int tid = threadIdx.x;
  if (tid < R) r_s[tid] = r[tid];
  if (tid < H) h_s[tid] = h[tid];
  for (int j = tid; j <= H; j += 128) dm[j] = (unsigned short)(j * WER_INS);
  for (int i = tid; i <= R; i += 128) dm[i * WER_LD] = (unsigned short)(i * WER_DEL);
  __syncthreads();
  const int i = tid + 1;
  for (int k = 2; k <= R + H; ++k) {
    const int j = k - i;
    if (i <= R && j >= 1 && j <= H) {
      int v = dm[(i - 1) * WER_LD + j - 1];
      if (r_s[i - 1] != h_s[j - 1])
        v = min(v + WER_SUB, min((int)dm[i * WER_LD + j - 1] + WER_INS, (int)dm[(i - 1) * WER_LD + j] + WER_DEL));
      dm[i * WER_LD + j] = (unsigned short)v;
    }
    lds_barrier();
  }
  if (tid == 0) {
    int xx = R, yy = H, nd = 0, ni = 0, ns = 0;
    for (int step = 0; step <= 3 * (R + H) && (xx > 0 || yy > 0); ++step) {
      const int v = dm[xx * WER_LD + yy];
      if (xx >= 1 && yy >= 1 && v == dm[(xx - 1) * WER_LD + yy - 1] && r_s[xx - 1] == h_s[yy - 1]) {
        --xx; --yy;
      } else if (xx >= 1 && yy >= 1 && v == dm[(xx - 1) * WER_LD + yy - 1] + WER_SUB) {
        ++ns; --xx; --yy;
      } else if (yy >= 1 && v == dm[xx * WER_LD + yy - 1] + WER_INS) {
        ++ni; --yy;
      } else {
        ++nd; xx = max(xx - 1, 0);
      }
    }
    out[0] = nd; out[1] = ni; out[2] = ns; out[3] = R;
  }
}

}  // namespace
