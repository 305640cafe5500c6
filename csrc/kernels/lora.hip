// Client-batched LoRA product for the fp32 LLaMA linears (models/lora.py, ops/lora.py): slot s is
// one client's adapter pair A[s] [r, D], B[s] [N, r] on a shared frozen base linear D -> N.
//
//   lora_fwd     u = x A^T  [S, T, r] (kept for the backward)  and  y += scale (u B^T)  in place
//   lora_bwd_x   v = scale (dy B)  [S, T, r]  and  dx (+)= v A   (dx optional)
//   lora_bwd_w   dA += v^T x,  dB += scale (dy^T u): per-chunk partials over T into a workspace,
//                folded in chunk order by lora_fold (no float atomics: same bits run to run)
//
// Everything is exact fp32 on v_mfma_f32_16x16x4_f32. A and B (dA, dB) are views into the
// [S, P] rows of the slot optimizer, so every launcher takes their slot stride; r in {4, 8, 16},
// D and N multiples of 16, any T >= 1 (rows past T are read as zero and never written).
// blockIdx.y (fwd / bwd_x) or .z (bwd_w, fold) is the slot: a slot's result depends on neither S
// nor the other slots' data.
//
// MFMA operand layout (lane = 16 g + c): first operand = M[i = c][k = g], second = M[k = g][j = c],
// result element e = D[i = 4 g + e][j = c]. All three products are formed TRANSPOSED (rank or
// feature index down the rows, token across the columns), so that
//   * a lane ends with 4 consecutive features of one token: one 16-byte access of y / dx / u / v;
//   * the rank-r intermediate of phase 1 (result layout) is already a valid second operand of
//     phase 2 with the reduction index k = 4 g + e, which the other operand simply follows: no
//     LDS transpose between the two products.
#include "ddl_common.h"

#define LORA_CHUNK 64  // tokens per reduction chunk of lora_bwd_w

__device__ __forceinline__ f4v ld4(const float* p) {
  const float4 v = *(const float4*)p;
  f4v r = {v.x, v.y, v.z, v.w};
  return r;
}
__device__ __forceinline__ f4v zero4() {
  f4v r = {0.f, 0.f, 0.f, 0.f};
  return r;
}

// The four waves' partial rank-r tiles summed in wave order; every wave gets the total.
__device__ __forceinline__ f4v fold_waves(f4v acc, f4v* lds, int wid, int lane) {
  lds[wid * 64 + lane] = acc;
  __syncthreads();
  f4v t = lds[lane];
#pragma unroll
  for (int w = 1; w < 4; ++w) t += lds[w * 64 + lane];
  return t;
}

// Block = 16 tokens of one slot, 4 waves. Phase 1: wave w reduces the 16-wide k chunks w, w + 4, ..
// of D; the partial tiles are summed in wave order through LDS. Phase 2: wave w takes the
// 16-column tiles w, w + 4, .. of N.
__global__ __launch_bounds__(256) void lora_fwd_kernel(const float* __restrict__ x,
                                                       const float* __restrict__ A,
                                                       const float* __restrict__ B,
                                                       float* __restrict__ y, float* __restrict__ u,
                                                       int T, int D, int N, int r, long long a_ss,
                                                       long long b_ss, float scale) {
  __shared__ f4v lds[4 * 64];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const int s = blockIdx.y, t = blockIdx.x * 16 + c;
  const bool tok = t < T;
  const long long row = (long long)s * T + (tok ? t : 0);
  const float* xs = x + row * D;
  const float* As = A + s * a_ss + (long long)c * D;
  const float* Bs = B + s * b_ss;
  f4v acc = zero4();
  for (int k = wid * 16 + 4 * g; k < D; k += 64) {
    const f4v xv = tok ? ld4(xs + k) : zero4();
    const f4v av = c < r ? ld4(As + k) : zero4();
#pragma unroll
    for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[e], xv[e], acc, 0, 0, 0);
  }
  const f4v uu = fold_waves(acc, lds, wid, lane);  // u[t][4 g + e]
  if (wid == 0 && tok && 4 * g < r) *(float4*)(u + row * r + 4 * g) = make_float4(uu[0], uu[1], uu[2], uu[3]);
  float* ys = y + row * N;
  for (int n0 = wid * 16; n0 < N; n0 += 64) {
    const f4v bv = 4 * g < r ? ld4(Bs + (long long)(n0 + c) * r + 4 * g) : zero4();
    f4v o = zero4();
#pragma unroll
    for (int e = 0; e < 4; ++e) o = __builtin_amdgcn_mfma_f32_16x16x4f32(bv[e], uu[e], o, 0, 0, 0);
    if (tok) {
      float4* dst = (float4*)(ys + n0 + 4 * g);
      float4 v = *dst;
      v.x += scale * o[0]; v.y += scale * o[1]; v.z += scale * o[2]; v.w += scale * o[3];
      *dst = v;
    }
  }
}

// Same shape as the forward with the roles turned: phase 1 reduces over N (v^T = B^T dy^T), phase
// 2 expands to D (dx^T = A^T v^T). dx == nullptr: the input needs no gradient, v is still made.
__global__ __launch_bounds__(256) void lora_bwd_x_kernel(const float* __restrict__ dy,
                                                         const float* __restrict__ A,
                                                         const float* __restrict__ B,
                                                         float* __restrict__ v, float* __restrict__ dx,
                                                         int T, int D, int N, int r, long long a_ss,
                                                         long long b_ss, float scale, int accumulate) {
  __shared__ f4v lds[4 * 64];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const int s = blockIdx.y, t = blockIdx.x * 16 + c;
  const bool tok = t < T;
  const long long row = (long long)s * T + (tok ? t : 0);
  const float* ds = dy + row * N;
  const float* As = A + s * a_ss;
  const float* Bs = B + s * b_ss;
  f4v acc = zero4();
  for (int n = wid * 16 + 4 * g; n < N; n += 64) {
    const f4v dv = tok ? ld4(ds + n) : zero4();
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float bv = c < r ? Bs[(long long)(n + e) * r + c] : 0.f;
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(bv, dv[e], acc, 0, 0, 0);
    }
  }
  f4v vv = fold_waves(acc, lds, wid, lane);  // v[t][4 g + e] before the scale
#pragma unroll
  for (int e = 0; e < 4; ++e) vv[e] *= scale;
  if (wid == 0 && tok && 4 * g < r) *(float4*)(v + row * r + 4 * g) = make_float4(vv[0], vv[1], vv[2], vv[3]);
  if (dx == nullptr) return;
  float* xs = dx + row * D;
  for (int d0 = wid * 16; d0 < D; d0 += 64) {
    f4v o = zero4();
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float av = 4 * g < r ? As[(long long)(4 * g + e) * D + d0 + c] : 0.f;
      o = __builtin_amdgcn_mfma_f32_16x16x4f32(av, vv[e], o, 0, 0, 0);
    }
    if (tok) {
      float4* dst = (float4*)(xs + d0 + 4 * g);
      float4 w = make_float4(o[0], o[1], o[2], o[3]);
      if (accumulate) {
        const float4 p = *dst;
        w.x += p.x; w.y += p.y; w.z += p.z; w.w += p.w;
      }
      *dst = w;
    }
  }
}

// One wave = 64 columns of x (dA) or dy (dB) x one chunk of LORA_CHUNK tokens of one slot:
// part[k][col] = sum_t small[t][k] big[t][col] with small = v (dA) or u (dB). Lane (c, g) reads the
// 16 bytes big[t0 + g][w0 + 4 c ..]: element q feeds accumulator tile q, whose column c is w0 + 4 c + q.
// Workspace per slot: [chunks][r D + r N], the dB part stored as [k][n].
__global__ __launch_bounds__(64) void lora_bwd_w_kernel(const float* __restrict__ x,
                                                        const float* __restrict__ dy,
                                                        const float* __restrict__ u,
                                                        const float* __restrict__ v,
                                                        float* __restrict__ ws, int T, int D, int N,
                                                        int r, int tiles_d, int want_da) {
  const int lane = threadIdx.x, c = lane & 15, g = lane >> 4;
  const int s = blockIdx.z, ch = blockIdx.y;
  int tile = blockIdx.x + (want_da ? 0 : tiles_d);
  const bool is_a = tile < tiles_d;
  if (!is_a) tile -= tiles_d;
  const int W = is_a ? D : N;
  const float* big = (is_a ? x : dy) + (long long)s * T * W;
  const float* small = (is_a ? v : u) + (long long)s * T * r;
  const int col = tile * 64 + 4 * c;
  const bool cok = col < W;
  const int t1 = min(T, (ch + 1) * LORA_CHUNK);
  f4v acc[4] = {zero4(), zero4(), zero4(), zero4()};
  for (int t = ch * LORA_CHUNK + g; t < t1 + g; t += 4) {  // uniform trip count over the wave
    const bool ok = t < t1;
    const f4v bv = ok && cok ? ld4(big + (long long)t * W + col) : zero4();
    const float sv = ok && c < r ? small[(long long)t * r + c] : 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(sv, bv[q], acc[q], 0, 0, 0);
  }
  const long long per = (long long)r * (D + N);
  float* part = ws + ((long long)s * gridDim.y + ch) * per + (is_a ? 0 : (long long)r * D);
  if (cok && 4 * g < r) {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      *(float4*)(part + (long long)(4 * g + e) * W + col) = make_float4(acc[0][e], acc[1][e], acc[2][e], acc[3][e]);
  }
}

// dA[s] += sum_ch partA[ch],  dB[s][n][k] += scale sum_ch partB[ch][k][n], chunks in ascending order.
__global__ __launch_bounds__(256) void lora_fold_kernel(const float* __restrict__ ws,
                                                        float* __restrict__ dA, float* __restrict__ dB,
                                                        int D, int N, int r, int chunks,
                                                        long long da_ss, long long db_ss, float scale) {
  const int s = blockIdx.y;
  const int na = r * D, nb = r * N;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= na + nb) return;
  const long long per = (long long)na + nb;
  const float* p = ws + (long long)s * chunks * per;
  if (i < na) {
    if (dA == nullptr) return;
    float t = p[i];
    for (int ch = 1; ch < chunks; ++ch) t += p[ch * per + i];
    dA[s * da_ss + i] += t;
  } else {
    const int j = i - na, n = j / r, k = j - n * r;
    const long long o = (long long)na + (long long)k * N + n;
    float t = p[o];
    for (int ch = 1; ch < chunks; ++ch) t += p[ch * per + o];
    dB[s * db_ss + j] += scale * t;
  }
}

static inline bool lora_shape_ok(int S, int T, int D, int N, int r) {
  return S >= 1 && S <= 65535 && T >= 1 && D >= 16 && N >= 16 && D % 16 == 0 && N % 16 == 0 &&
         (r == 4 || r == 8 || r == 16);
}

DDL_API int ddl_lora_chunk() { return LORA_CHUNK; }

// floats of workspace one slot of lora_bwd_w needs
DDL_API long long ddl_lora_workspace(int T, int D, int N, int r) {
  return (long long)((T + LORA_CHUNK - 1) / LORA_CHUNK) * r * (D + N);
}

DDL_API int ddl_lora_fwd(const float* x, const float* A, const float* B, float* y, float* u, int S,
                         int T, int D, int N, int r, long long a_ss, long long b_ss, float scale,
                         hipStream_t st) {
  if (!lora_shape_ok(S, T, D, N, r) || !x || !A || !B || !y || !u) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(lora_fwd_kernel, dim3((T + 15) / 16, S), dim3(256), 0, st, x, A, B, y, u, T, D, N,
                     r, a_ss, b_ss, scale);
  return (int)hipGetLastError();
}

DDL_API int ddl_lora_bwd_x(const float* dy, const float* A, const float* B, float* v, float* dx, int S,
                           int T, int D, int N, int r, long long a_ss, long long b_ss, float scale,
                           int accumulate, hipStream_t st) {
  if (!lora_shape_ok(S, T, D, N, r) || !dy || !A || !B || !v) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(lora_bwd_x_kernel, dim3((T + 15) / 16, S), dim3(256), 0, st, dy, A, B, v, dx, T, D,
                     N, r, a_ss, b_ss, scale, accumulate);
  return (int)hipGetLastError();
}

// dA == nullptr (A frozen): the v^T x product is skipped, its workspace part stays unwritten.
DDL_API int ddl_lora_bwd_w(const float* x, const float* dy, const float* u, const float* v, float* dA,
                           float* dB, float* ws, int S, int T, int D, int N, int r, long long da_ss,
                           long long db_ss, float scale, hipStream_t st) {
  if (!lora_shape_ok(S, T, D, N, r) || !dy || !u || !dB || !ws || (dA && (!x || !v)))
    return (int)hipErrorInvalidValue;
  const int chunks = (T + LORA_CHUNK - 1) / LORA_CHUNK;
  if (chunks > 65535) return (int)hipErrorInvalidValue;
  const int tiles_d = (D + 63) / 64, tiles_n = (N + 63) / 64;
  hipLaunchKernelGGL(lora_bwd_w_kernel, dim3((dA ? tiles_d : 0) + tiles_n, chunks, S), dim3(64), 0, st, x,
                     dy, u, v, ws, T, D, N, r, tiles_d, dA ? 1 : 0);
  int rc = (int)hipGetLastError();
  if (rc) return rc;
  hipLaunchKernelGGL(lora_fold_kernel, dim3((r * (D + N) + 255) / 256, S), dim3(256), 0, st, ws, dA, dB, D,
                     N, r, chunks, da_ss, db_ss, scale);
  return (int)hipGetLastError();
}
