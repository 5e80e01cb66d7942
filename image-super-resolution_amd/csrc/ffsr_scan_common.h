// Pieces shared by the two selective-scan files: ffsr_scan.hip (fused 4-direction, pixel-major) and ffsr_scan_seq.hip
// (mamba_ssm's selective_scan_fn on the channel-major [B, D, L] layout).  Both cut the sequence into chunks and run the
// same three passes; the carry over chunks (pass B) and the softplus of delta are identical, so they live here.
#pragma once
#include "ffsr_common.h"

namespace {

// softplus with torch's threshold 20, on the hardware exp2/log2: log1p(e) = e(1 - e(1/2 - e/3)) for small e = exp(x)
// (relative error < 4e-7), log(1 + e) otherwise.  Branch-free selects.
__device__ __forceinline__ float softplus_f(float x) {
  const float e = __builtin_amdgcn_exp2f(fminf(x, 20.f) * 1.4426950408889634f);
  const float small = e * (1.f - e * (0.5f - e * 0.33333334f));
  const float big = __builtin_amdgcn_logf(1.f + e) * 0.6931471805599453f;
  const float sp = e < 0.01f ? small : big;
  return x > 20.f ? x : sp;
}

// hstate[c] <- state entering chunk c.  The carry over chunks is the affine recurrence h' = decay * h + local, one
// independent chain per (batch, [direction,] channel, state) = only B*4*Dm*16 chains (fused scan): a thread per chain walks ~512
// chunks with dependent loads on a quarter of the chip.  Here a 1024-thread block covers 64 chains x SEG = 16 segments
// of the chunk range: every thread composes the affine map of its segment (h -> P h + Q), the 16 maps are combined
// through LDS, and the segment is walked a second time from its true incoming state.  Lanes run along the chains, so
// every access is a contiguous 256-byte row segment.
constexpr int CARRY_SEG = 16;
__global__ __launch_bounds__(64 * CARRY_SEG) void scan_carry_kernel(float* __restrict__ hstate, const float* __restrict__ decay,
                                                                    int nchunk, int per) {
  __shared__ float Ps[CARRY_SEG][64], Qs[CARRY_SEG][64];
  const int lane = threadIdx.x & 63, seg = threadIdx.x >> 6;
  const int i = blockIdx.x * 64 + lane, g = blockIdx.y;
  const bool live = i < per;
  const int ii = live ? i : per - 1;
  const int cps = (nchunk + CARRY_SEG - 1) / CARRY_SEG;
  const int c0 = seg * cps, c1 = min(nchunk, c0 + cps);
  const size_t base = (size_t)g * nchunk * per + ii;
  float P = 1.f, Q = 0.f;
  constexpr int U = 8;  // loads of U chunks are issued together (they do not depend on the recurrence)
  for (int cc = c0; cc < c1; cc += U) {
    float hl[U], dc[U];
#pragma unroll
    for (int j = 0; j < U; ++j) {
      const size_t o = base + (size_t)min(cc + j, nchunk - 1) * per;
      hl[j] = hstate[o];
      dc[j] = decay[o];
    }
#pragma unroll
    for (int j = 0; j < U; ++j)
      if (cc + j < c1) {
        P *= dc[j];
        Q = fmaf(dc[j], Q, hl[j]);
      }
  }
  Ps[seg][lane] = P;
  Qs[seg][lane] = Q;
  __syncthreads();
  float hin = 0.f;
  for (int sgm = 0; sgm < seg; ++sgm) hin = fmaf(Ps[sgm][lane], hin, Qs[sgm][lane]);
  for (int cc = c0; cc < c1; cc += U) {
    float hl[U], dc[U];
#pragma unroll
    for (int j = 0; j < U; ++j) {
      const size_t o = base + (size_t)min(cc + j, nchunk - 1) * per;
      hl[j] = hstate[o];
      dc[j] = decay[o];
    }
#pragma unroll
    for (int j = 0; j < U; ++j)
      if (cc + j < c1) {
        if (live) hstate[base + (size_t)(cc + j) * per] = hin;
        hin = fmaf(dc[j], hin, hl[j]);
      }
  }
}

}  // namespace
