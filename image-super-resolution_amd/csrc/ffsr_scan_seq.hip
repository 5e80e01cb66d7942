// mamba_ssm's selective_scan_fn (forward) on its own channel-major layouts, gfx950: the seam MambaIR's SS2D binds as
// `self.selective_scan = selective_scan_fn` (mambair_arch.py:276, called at :356-362).
//
//   delta_t = softplus?(delta[b,d,t] + delta_bias[d])
//   h_t[n]  = exp(delta_t * A[d,n]) * h_{t-1}[n] + delta_t * B[b,g(d),n,t] * u[b,d,t]
//   y_t     = sum_n C[b,g(d),n,t] * h_t[n] + D[d] * u[b,d,t];   y *= silu(z[b,d,t]) if z is given
//
// u, delta, z, y: [B, Dm, L]; B, C: [B, G, N, L] (channel d in group d / (Dm/G)); last dimension unit-stride.
//
// Same three passes as ffsr_scan.hip (lane = channel, N states in registers; pass A: local chunk end state and decay,
// pass B: scan_carry_kernel, pass C: re-run from the true incoming state and emit y; the last chunk's pass C writes
// last_state).  What is new is the memory side: along a channel the sequence is contiguous, so a lane-per-channel read of
// u[b, d, t] per step would be a 64-way strided gather.  Instead, per group of T steps, [64 channels x T steps] tiles of
// u, delta and z are loaded with 16-byte loads along L (two lanes per channel row), written transposed into LDS and read
// back with lane = channel; y goes out the same way through the u tile (each lane overwrites only its own column).  The
// group's B / C rows are wave-uniform (a workgroup's channels lie in one group) and are read as LDS broadcasts.  As in
// ffsr_scan.hip the next group is fetched into registers while the current one runs, so the recurrence does not wait on
// HBM.  LDS is one 7.9 KB buffer per wave, leaving the 4 waves / SIMD the VALU-bound recurrence wants.
#include "ffsr_common.h"
#include "ffsr_scan_common.h"

namespace {

constexpr int T = 8;    // steps per group
constexpr int TS = 72;  // LDS row stride of a [T][64] tile: 4 * TS % 64 == 32 makes the transposing writes conflict-free

struct SeqArgs {
  const float* u;
  const float* delta;
  const float* A;      // [Dm, N]
  const float* Bm;     // [B, G, N, L], row stride L
  const float* Cm;
  const float* Dv;     // [Dm] or null
  const float* z;      // or null
  const float* dbias;  // [Dm] or null
  float* y;            // [B, Dm, L] contiguous
  float* last;         // [B, Dm, N] or null
  float* hstate;       // [B, nchunk, Dm, N]
  float* decay;
  long long su_b, su_d, sdt_b, sdt_d, sz_b, sz_d, sbc_b, sbc_g;
  int Dm, L, rep, nbg, softplus, chunk, nchunk;
};

// 4 consecutive steps t..t+3 of one row (zeros past L or for a null row).  VEC: 16-byte aligned rows and L % 4 == 0, so a
// vector is either wholly inside the sequence or wholly past it.
template <bool VEC>
__device__ __forceinline__ floatx4 load4(const float* row, int t, int L) {
  floatx4 v = {0.f, 0.f, 0.f, 0.f};
  if (!row) return v;
  if (VEC) {
    if (t < L) v = *reinterpret_cast<const floatx4*>(row + t);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (t + j < L) v[j] = row[t + j];
  }
  return v;
}

template <bool VEC>
__device__ __forceinline__ void store4(float* row, int t, int L, floatx4 v) {
  if (VEC) {
    if (t < L) *reinterpret_cast<floatx4*>(row + t) = v;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (t + j < L) row[t + j] = v[j];
  }
}

// grid (G * nbg, nchunk, B): block x = (group g, channel block j of that group), 64 lanes = channels g*rep + 64j + lane.
// Tile loader mapping: element i of lane l (i = 0, 1) is channel row (l >> 1) + 32 i, steps 4 (l & 1) .. + 3 of the group;
// B / C rows: lane l < 2N loads B row l >> 1, lanes 2N .. 4N-1 the C rows (pass C only), steps 4 (l & 1) .. + 3.
template <int N, bool EMIT, bool HAS_Z, bool VEC>
__global__ __launch_bounds__(64, 4) void seq_scan_chunk_kernel(SeqArgs p) {
  __shared__ float us[T * TS], ds[T * TS], zs[HAS_Z ? T * TS : 1];
  __shared__ float bs[T * N], cs[EMIT ? T * N : 1];
  const int lane = threadIdx.x;
  const int g = blockIdx.x / p.nbg, jb = blockIdx.x - g * p.nbg;
  const int c0 = g * p.rep + jb * 64;                 // first channel of the block
  const int nlive = min(64, p.rep - jb * 64);
  const int c = blockIdx.y, b = blockIdx.z;
  const bool live = lane < nlive;
  const int d = c0 + (live ? lane : 0);
  float a2[N], h[N];
  const size_t sidx = (((size_t)b * p.nchunk + c) * p.Dm + d) * N;
#pragma unroll
  for (int n = 0; n < N; ++n) {
    a2[n] = p.A[(size_t)d * N + n] * 1.4426950408889634f;  // exp(x) = 2^(x log2 e)
    h[n] = EMIT ? p.hstate[sidx + n] : 0.f;
  }
  const float bias = p.dbias ? p.dbias[d] : 0.f;
  const float dskip = p.Dv ? p.Dv[d] : 0.f;
  const int t0 = c * p.chunk, t1 = min(p.L, t0 + p.chunk);

  // per-lane source rows of the tile loader (null = channel row past the block's live channels: loads zeros)
  const int tq = 4 * (lane & 1);
  const float *urow[2], *drow[2], *zrow[2];
  float* yrow[2];
  int tcol[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int ch = (lane >> 1) + 32 * i;
    const bool ok = ch < nlive;
    const long long dc = c0 + ch;
    tcol[i] = ch;
    urow[i] = ok ? p.u + b * p.su_b + dc * p.su_d : nullptr;
    drow[i] = ok ? p.delta + b * p.sdt_b + dc * p.sdt_d : nullptr;
    zrow[i] = (HAS_Z && ok) ? p.z + b * p.sz_b + dc * p.sz_d : nullptr;
    yrow[i] = ok ? p.y + ((size_t)b * p.Dm + dc) * p.L : nullptr;
  }
  const float* bcrow = nullptr;
  if (lane < 2 * N)
    bcrow = p.Bm + b * p.sbc_b + g * p.sbc_g + (size_t)(lane >> 1) * p.L;
  else if (EMIT && lane < 4 * N)
    bcrow = p.Cm + b * p.sbc_b + g * p.sbc_g + (size_t)((lane - 2 * N) >> 1) * p.L;

  floatx4 un[2], dn[2], zn[2], bcn;
  auto fetch = [&](int tg) {  // global -> registers for the group starting at step tg
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      un[i] = load4<VEC>(urow[i], tg + tq, p.L);
      dn[i] = load4<VEC>(drow[i], tg + tq, p.L);
      if (HAS_Z) zn[i] = load4<VEC>(zrow[i], tg + tq, p.L);
    }
    bcn = load4<VEC>(bcrow, tg + tq, p.L);
  };
  auto commit = [&]() {  // registers -> LDS, transposed to [step][channel] and [step][state]
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        us[(tq + j) * TS + tcol[i]] = un[i][j];
        ds[(tq + j) * TS + tcol[i]] = dn[i][j];
        if (HAS_Z) zs[(tq + j) * TS + tcol[i]] = zn[i][j];
      }
    if (lane < 2 * N) {
#pragma unroll
      for (int j = 0; j < 4; ++j) bs[(tq + j) * N + (lane >> 1)] = bcn[j];
    } else if (EMIT && lane < 4 * N) {
#pragma unroll
      for (int j = 0; j < 4; ++j) cs[(tq + j) * N + ((lane - 2 * N) >> 1)] = bcn[j];
    }
  };
  fetch(t0);
  commit();
  __syncthreads();
  float dsum = 0.f;
  for (int tg = t0; tg < t1; tg += T) {
    const bool more = tg + T < t1;
    if (more) fetch(tg + T);
#pragma unroll
    for (int r = 0; r < T; ++r) {
      if (tg + r < t1) {
        const float uu = us[r * TS + lane];
        float dl = ds[r * TS + lane] + bias;
        if (p.softplus) dl = softplus_f(dl);
        const float du = dl * uu;
        const float* br = bs + r * N;  // wave-uniform LDS reads (broadcast)
        float yv = 0.f;
#pragma unroll
        for (int n = 0; n < N; ++n) {
          const float dA = __builtin_amdgcn_exp2f(dl * a2[n]);
          h[n] = fmaf(dA, h[n], du * br[n]);
          if (EMIT) yv = fmaf(cs[r * N + n], h[n], yv);
        }
        if (EMIT) {
          float yo = fmaf(dskip, uu, yv);
          if (HAS_Z) {
            const float zz = zs[r * TS + lane];
            yo *= zz / (1.f + __builtin_amdgcn_exp2f(-zz * 1.4426950408889634f));
          }
          us[r * TS + lane] = yo;  // the lane's own column: no other lane touches it before the barrier
        } else {
          dsum += dl;
        }
      }
    }
    if (EMIT) {  // y tile out along L, then the tile is free for the next group
      __syncthreads();
#pragma unroll
      for (int i = 0; i < 2; ++i)
        if (yrow[i]) {
          floatx4 v;
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] = us[(tq + j) * TS + tcol[i]];
          store4<VEC>(yrow[i], tg + tq, t1, v);
        }
      __syncthreads();
    }
    if (more) commit();
    __syncthreads();
  }
  if (!live) return;
  if (!EMIT) {
#pragma unroll
    for (int n = 0; n < N; ++n) {
      p.hstate[sidx + n] = h[n];
      p.decay[sidx + n] = __builtin_amdgcn_exp2f(a2[n] * dsum);
    }
  } else if (p.last && c == p.nchunk - 1) {
#pragma unroll
    for (int n = 0; n < N; ++n) p.last[((size_t)b * p.Dm + d) * N + n] = h[n];
  }
}

template <int N, bool VEC>
int run_seq_scan(const SeqArgs& a, int Bsz, int G, hipStream_t st) {
  dim3 grid(G * a.nbg, a.nchunk, Bsz);
  FFSR_LAUNCH((seq_scan_chunk_kernel<N, false, false, VEC>), grid, dim3(64), 0, st, a);
  FFSR_LAUNCH(scan_carry_kernel, dim3((a.Dm * N + 63) / 64, Bsz), dim3(64 * CARRY_SEG), 0, st, a.hstate, a.decay, a.nchunk,
              a.Dm * N);
  if (a.z)
    FFSR_LAUNCH((seq_scan_chunk_kernel<N, true, true, VEC>), grid, dim3(64), 0, st, a);
  else
    FFSR_LAUNCH((seq_scan_chunk_kernel<N, true, false, VEC>), grid, dim3(64), 0, st, a);
  return ffsr_launch_status();
}

template <int N>
int run_seq_scan_n(const SeqArgs& a, bool vec, int Bsz, int G, hipStream_t st) {
  return vec ? run_seq_scan<N, true>(a, Bsz, G, st) : run_seq_scan<N, false>(a, Bsz, G, st);
}

}  // namespace

extern "C" int ffsr_selective_scan_f32(const float* u, const float* delta, const float* A, const float* Bm, const float* Cm,
                                       const float* D, const float* z, const float* delta_bias, float* y, float* last_state,
                                       float* hstate, float* decay, long long su_b, long long su_d, long long sdt_b,
                                       long long sdt_d, long long sz_b, long long sz_d, long long sbc_b, long long sbc_g,
                                       int Bsz, int Dm, int L, int N, int G, int softplus, int chunk, void* stream) {
  FFSR_CHECK(u && delta && A && Bm && Cm && y && hstate && decay);
  FFSR_CHECK(N == 16 || N == 8);
  FFSR_CHECK(Bsz > 0 && Dm > 0 && L > 0 && G > 0 && Dm % G == 0 && chunk > 0 && chunk % T == 0);
  SeqArgs a;
  a.u = u; a.delta = delta; a.A = A; a.Bm = Bm; a.Cm = Cm; a.Dv = D; a.z = z; a.dbias = delta_bias; a.y = y;
  a.last = last_state; a.hstate = hstate; a.decay = decay;
  a.su_b = su_b; a.su_d = su_d; a.sdt_b = sdt_b; a.sdt_d = sdt_d; a.sz_b = sz_b; a.sz_d = sz_d; a.sbc_b = sbc_b;
  a.sbc_g = sbc_g;
  a.Dm = Dm; a.L = L; a.rep = Dm / G; a.nbg = (a.rep + 63) / 64; a.softplus = softplus != 0; a.chunk = chunk;
  a.nchunk = (L + chunk - 1) / chunk;
  FFSR_CHECK(a.nchunk <= 65535 && Bsz <= 65535 && (long long)G * a.nbg <= 0x7fffffffLL);
  auto al = [](const void* q) { return ((uintptr_t)q & 15) == 0; };
  const bool vec = L % 4 == 0 && al(u) && al(delta) && al(Bm) && al(Cm) && al(y) && (!z || al(z)) &&
                   ((su_b | su_d | sdt_b | sdt_d | sbc_b | sbc_g) & 3) == 0 && (!z || ((sz_b | sz_d) & 3) == 0);
  hipStream_t st = (hipStream_t)stream;
  return N == 16 ? run_seq_scan_n<16>(a, vec, Bsz, G, st) : run_seq_scan_n<8>(a, vec, Bsz, G, st);
}
