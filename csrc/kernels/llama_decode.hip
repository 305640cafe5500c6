// Text generation for the fp32 tiny LLaMA: the decode step's own short chain of kernels (all
// gfx950, fp32 in and out, deterministic: no float atomics, every reduction in a fixed order).
// The training linears are built for T in the hundreds (128-row tiles, a plane split per call,
// plan-table lookups); a decode step has 1..16 rows and is bound by launches and latency.
//
//   ddl_lin_rows_f32     y[T,K] = pro(x)[T,C] W[K,C]^T (+ residual), 1 <= T <= 16: W streamed once, a
//                        wave per output column (four on wide outputs), x staged once per workgroup
//                        in LDS with the prologue applied while staging (none | rmsnorm | swiglu),
//                        an fmaf chain per lane and one xor-butterfly wave reduction
//   ddl_lora_rows_u      per-sequence adapters (row t uses adapter ids[t]; an id out of range = none):
//   ddl_lin_rows_lora_f32  the shrink u = pro(x) A[ids[t]]^T on the rows lin_rows stages, one workgroup
//                        per row; the expand y += scale u B[ids[t]]^T in lin_rows' own epilogue
//   ddl_attnf_decode     single-query attention over one layer's cache [B][H][Smax][HD] (K stored
//                        rotated) with the step's K / V row appended by split 0 of the same launch;
//                        grid (H, B, NS), NS fixed from Smax on the host so the launch is capturable;
//                        four lanes per key, an online softmax per quad, quads merged by a butterfly,
//                        waves through LDS in wave order; NS > 1 writes per-split records that
//                        ddl_attnf_decode's second kernel merges in split order
//   ddl_kv_append        prefill: rotate K at absolute positions and write K / V rows into the cache
//   ddl_sample_f32       one workgroup per row: argmax (temperature 0) or temperature / top-k sampling
//                        (exact 4 x 8-bit radix select on the logits, ties by lowest index), inverse
//                        CDF in vocabulary order with a Philox uniform; also the step's state update
//                        (next token, output column, lens, finished, step counter), so nothing a
//                        step needs for the next one leaves the device
//
// Sequence state: lens[b] = rows of sequence b in the cache. A sequence with lens[b] outside
// [0, Smax) is FROZEN: the attention stores nothing, reads nothing and returns zeros, the sampler
// leaves its lens alone. No index is formed from lens before that test.
#include "ddl_common.h"

#include <limits.h>

namespace {

constexpr float DEC_LOG2E = 1.4426950408889634f;

__device__ __forceinline__ float dec_quad_sum(float v) {  // the 4 lanes of a quad, same bits in each
  v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0xB1, 0xF, 0xF, true));  // [1,0,3,2]
  v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x4E, 0xF, 0xF, true));  // [2,3,0,1]
  return v;
}
template <int N>
__device__ __forceinline__ void dec_load(const float* p, float (&v)[N]) {
#pragma unroll
  for (int m = 0; m < N; m += 4) {
    const float4 f = *(const float4*)(p + m);
    v[m] = f.x; v[m + 1] = f.y; v[m + 2] = f.z; v[m + 3] = f.w;
  }
}
template <int N>
__device__ __forceinline__ void dec_store(float* p, const float (&v)[N]) {
#pragma unroll
  for (int m = 0; m < N; m += 4) *(float4*)(p + m) = make_float4(v[m], v[m + 1], v[m + 2], v[m + 3]);
}
// rotate dims d0.. of a row (interleaved pairs; cs / sn = the position's table rows)
template <int N>
__device__ __forceinline__ void dec_rope(float (&v)[N], const float* cs, const float* sn, int d0) {
#pragma unroll
  for (int m = 0; m < N; m += 2) {
    const float c = cs[(d0 + m) >> 1], s = sn[(d0 + m) >> 1];
    const float a = v[m], b = v[m + 1];
    v[m] = a * c - b * s;
    v[m + 1] = a * s + b * c;
  }
}
template <int N>
__device__ __forceinline__ float dec_dot(const float (&a)[N], const float (&b)[N]) {
  float s = 0.f;
#pragma unroll
  for (int m = 0; m < N; ++m) s = fmaf(a[m], b[m], s);
  return s;
}
__device__ __forceinline__ float dec_sigm(float a) { return 1.f / (1.f + expf(-a)); }
// weight of a partial softmax record with maximum m under the merged maximum nm (an empty record
// has m = -inf and weight 0, also when nm = -inf)
__device__ __forceinline__ float dec_w(float m, float nm) { return m == -INFINITY ? 0.f : exp2f(m - nm); }

}  // namespace

// ---------------------------------------------------------------------------------------------
// Skinny-row linear. Workgroup = 4 waves; wave w owns output columns k0 + R w .. + R - 1. LDS holds
// TT >= T rows of pro(x) (rows >= T zero). Lane l reads float4 chunk l, l + 64, .. of a W row and
// of every staged row: acc[r][t] is an fmaf chain over the lane's chunks, then the wave butterfly.
constexpr int LR_MAX_T = 16, LR_LDS_BYTES = 65536, LR_RMS_MAXV = 8;
enum { LR_NONE = 0, LR_RMS = 1, LR_SWIGLU = 2 };

// pro(x) rows 0 .. TT - 1 into LDS (rows >= T zero), by the whole workgroup; x rows are xs floats
// apart. The one staging routine of every kernel here that reads pro(x): their staged bits agree.
template <int TT>
__device__ __forceinline__ void lr_stage(const float* __restrict__ x, const float* __restrict__ gain, float4* xs4,
                                         int T, int C, int pro, float eps) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int C4 = C / 4;
  if (pro == LR_RMS) {
    // a wave per row, as ddl_rmsf_fwd: the lane's slices in registers, the same sums and products
    for (int t = wv; t < TT; t += 4) {
      float4 v[LR_RMS_MAXV];
      float ss = 0.f;
      const float4* xr = (const float4*)(x + (long long)t * C);
#pragma unroll
      for (int k = 0; k < LR_RMS_MAXV; ++k) {
        const int c = lane + 64 * k;
        v[k] = (t < T && c < C4) ? xr[c] : make_float4(0.f, 0.f, 0.f, 0.f);
        ss += v[k].x * v[k].x + v[k].y * v[k].y + v[k].z * v[k].z + v[k].w * v[k].w;
      }
      ss = wave_sum(ss);
      const float r = 1.f / sqrtf(ss / (float)C + eps);
      const float4* g4 = (const float4*)gain;
#pragma unroll
      for (int k = 0; k < LR_RMS_MAXV; ++k) {
        const int c = lane + 64 * k;
        if (c < C4) {
          const float4 gg = g4[c];
          xs4[t * C4 + c] = make_float4(v[k].x * r * gg.x, v[k].y * r * gg.y, v[k].z * r * gg.z, v[k].w * r * gg.w);
        }
      }
    }
  } else {
    for (int e = threadIdx.x; e < TT * C4; e += 256) {
      const int t = e / C4, c = e - t * C4;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (t < T) {
        if (pro == LR_SWIGLU) {
          const float4 a = ((const float4*)(x + (long long)t * 2 * C))[c];
          const float4 b = ((const float4*)(x + (long long)t * 2 * C + C))[c];
          v = make_float4(a.x * dec_sigm(a.x) * b.x, a.y * dec_sigm(a.y) * b.y, a.z * dec_sigm(a.z) * b.z,
                          a.w * dec_sigm(a.w) * b.w);
        } else {
          v = ((const float4*)(x + (long long)t * C))[c];
        }
      }
      xs4[e] = v;
    }
  }
}

// The adapters of a decode step (multi-LoRA serving: row t of the batch uses adapter ids[t]).
// u [T][r] = pro(x) A[ids[t]]^T comes from ddl_lora_rows_u; B [Rn][K][r], slots bs floats apart.
// An id outside [0, Rn) means "no adapter": no index is formed from it.
struct LrLora {
  const float* u;
  const float* B;
  const int* ids;
  long long bs;
  int Rn, r;
  float scale;
};

// the LoRA term of output (t, k): an fmaf chain over j ascending from 0
__device__ __forceinline__ float lr_delta(const LrLora& lo, int id, int t, int k) {
  const float4* u4 = (const float4*)(lo.u + (long long)t * lo.r);
  const float4* b4 = (const float4*)(lo.B + (long long)id * lo.bs + (long long)k * lo.r);
  float d = 0.f;
  for (int j = 0; j < lo.r / 4; ++j) {
    const float4 uv = u4[j], bv = b4[j];
    d = fmaf(uv.x, bv.x, d);
    d = fmaf(uv.y, bv.y, d);
    d = fmaf(uv.z, bv.z, d);
    d = fmaf(uv.w, bv.w, d);
  }
  return d;
}

template <int TT, int R, bool LORA>
__global__ __launch_bounds__(256) void lin_rows_f32_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                           const float* __restrict__ res,
                                                           const float* __restrict__ gain, float* __restrict__ y,
                                                           int T, int C, int K, int pro, float eps, LrLora lo) {
  extern __shared__ __attribute__((aligned(16))) float lr_xs[];  // [TT][C]
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int C4 = C / 4;
  float4* xs4 = (float4*)lr_xs;
  int id = -1;  // lane t owns row t's outputs: its adapter, read ahead of the W stream
  if (LORA && lane < T) {
    id = lo.ids[lane];
    if (id < 0 || id >= lo.Rn) id = -1;
  }
  lr_stage<TT>(x, gain, xs4, T, C, pro, eps);
  __syncthreads();
  const int k0 = (blockIdx.x * 4 + wv) * R;
  if (k0 >= K) return;
  float acc[R][TT];
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int t = 0; t < TT; ++t) acc[r][t] = 0.f;
  for (int c = lane; c < C4; c += 64) {
    float4 wr[R];
#pragma unroll
    for (int r = 0; r < R; ++r)
      wr[r] = ((const float4*)(w + (long long)min(k0 + r, K - 1) * C))[c];  // clamped row: computed, not stored
#pragma unroll
    for (int t = 0; t < TT; ++t) {
      const float4 xv = xs4[t * C4 + c];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        float a = acc[r][t];
        a = fmaf(wr[r].x, xv.x, a);
        a = fmaf(wr[r].y, xv.y, a);
        a = fmaf(wr[r].z, xv.z, a);
        a = fmaf(wr[r].w, xv.w, a);
        acc[r][t] = a;
      }
    }
  }
  if (LORA) {
    // every lane keeps its own row's sums, then the T owning lanes run their epilogues side by side:
    // one round of u / B / residual loads for the wave, not one per row
#pragma unroll
    for (int r = 0; r < R; ++r) {
      float mine = 0.f;
#pragma unroll
      for (int t = 0; t < TT; ++t) {
        const float s = wave_sum(acc[r][t]);
        if (lane == t) mine = s;
      }
      const int k = k0 + r;
      if (lane < T && k < K) {
        const long long at = (long long)lane * K + k;
        if (id >= 0) mine = fmaf(lo.scale, lr_delta(lo, id, lane, k), mine);  // no adapter: the sum as it is
        y[at] = res ? mine + res[at] : mine;
      }
    }
    return;
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
#pragma unroll
    for (int t = 0; t < TT; ++t) {
      const float s = wave_sum(acc[r][t]);
      const int k = k0 + r;
      if (lane == t && t < T && k < K) {
        const long long at = (long long)t * K + k;
        y[at] = res ? s + res[at] : s;
      }
    }
  }
}

template <int TT, bool LORA>
static int lin_rows_launch(const float* x, const float* w, const float* res, const float* gain, float* y, int T,
                           int C, int K, int pro, float eps, const LrLora& lo, hipStream_t s) {
  const size_t lds = (size_t)TT * C * sizeof(float);
  if (lds > (size_t)LR_LDS_BYTES) return (int)hipErrorInvalidValue;
  if (K > 4096) {  // wide outputs (the LM head): four columns per wave, four W rows in flight per lane
    hipLaunchKernelGGL((lin_rows_f32_kernel<TT, 4, LORA>), dim3((K + 15) / 16), dim3(256), lds, s, x, w, res, gain, y,
                       T, C, K, pro, eps, lo);
  } else {
    hipLaunchKernelGGL((lin_rows_f32_kernel<TT, 1, LORA>), dim3((K + 3) / 4), dim3(256), lds, s, x, w, res, gain, y,
                       T, C, K, pro, eps, lo);
  }
  return (int)hipGetLastError();
}

static bool lin_rows_args_ok(const float* x, const float* w, const float* gain, const float* y, int T, int C, int K,
                             int pro) {
  if (!x || !w || !y || T < 1 || T > LR_MAX_T || C < 4 || C % 4 || K < 1) return false;
  if (pro != LR_NONE && pro != LR_RMS && pro != LR_SWIGLU) return false;
  if (pro == LR_RMS && (!gain || C > 256 * LR_RMS_MAXV)) return false;
  return true;
}

template <bool LORA>
static int lin_rows_dispatch(const float* x, const float* w, const float* res, const float* gain, float* y, int T,
                             int C, int K, int pro, float eps, const LrLora& lo, hipStream_t s) {
  if (T == 1) return lin_rows_launch<1, LORA>(x, w, res, gain, y, T, C, K, pro, eps, lo, s);
  if (T == 2) return lin_rows_launch<2, LORA>(x, w, res, gain, y, T, C, K, pro, eps, lo, s);
  if (T <= 4) return lin_rows_launch<4, LORA>(x, w, res, gain, y, T, C, K, pro, eps, lo, s);
  if (T <= 8) return lin_rows_launch<8, LORA>(x, w, res, gain, y, T, C, K, pro, eps, lo, s);
  return lin_rows_launch<16, LORA>(x, w, res, gain, y, T, C, K, pro, eps, lo, s);
}

// x [T][C] ([T][2C] = [a | b] for the swiglu prologue), w [K][C], res / y [T][K]; gain [C] for the
// rmsnorm prologue (C <= 2048 there, as ddl_rmsf_fwd). The staged rows must fit 64 KB of LDS.
DDL_API int ddl_lin_rows_f32(const float* x, const float* w, const float* res, const float* gain, float* y, int T,
                             int C, int K, int pro, float eps, hipStream_t s) {
  if (!lin_rows_args_ok(x, w, gain, y, T, C, K, pro)) return (int)hipErrorInvalidValue;
  return lin_rows_dispatch<false>(x, w, res, gain, y, T, C, K, pro, eps, LrLora{}, s);
}

static bool lr_al16(const void* p) { return ((uintptr_t)p & 15u) == 0; }
static bool lr_rank_ok(int r) { return r == 4 || r == 8 || r == 16; }

// ddl_lin_rows_f32 with the adapter's expand fused into the epilogue: the lane that owns (t, k) adds
// scale * sum_j u[t][j] B[ids[t]][k][j] to the reduced sum before the residual. u [T][r] (16-byte
// aligned), B [Rn][K][r] with slots b_stride floats apart, ids int32 [T]. A row whose id is outside
// [0, Rn) takes ddl_lin_rows_f32's own expression and has its bits.
DDL_API int ddl_lin_rows_lora_f32(const float* x, const float* w, const float* res, const float* gain, float* y,
                                  int T, int C, int K, int pro, float eps, const float* u, const float* B,
                                  const int* ids, int Rn, long long b_stride, int r, float scale, hipStream_t s) {
  if (!lin_rows_args_ok(x, w, gain, y, T, C, K, pro)) return (int)hipErrorInvalidValue;
  if (!u || !B || !ids || Rn < 1 || !lr_rank_ok(r) || !lr_al16(u) || !lr_al16(B)) return (int)hipErrorInvalidValue;
  if (b_stride % 4 || (Rn > 1 && b_stride < (long long)K * r)) return (int)hipErrorInvalidValue;
  const LrLora lo{u, B, ids, b_stride, Rn, r, scale};
  return lin_rows_dispatch<true>(x, w, res, gain, y, T, C, K, pro, eps, lo, s);
}

// The adapter's shrink: u[t][j] = pro(x)[t] . A[ids[t]][j]. One workgroup per row: the row staged by
// lr_stage (the bits ddl_lin_rows_f32 stages), wave w takes ranks w, w + 4, ..; each lane an fmaf
// chain over its float4 chunks, then the wave butterfly. No adapter: the row of u is zero.
template <int NR>
__global__ __launch_bounds__(256) void lora_rows_u_kernel(const float* __restrict__ x, const float* __restrict__ A,
                                                          const int* __restrict__ ids,
                                                          const float* __restrict__ gain, float* __restrict__ u,
                                                          int C, int Rn, long long as, int pro, float eps) {
  extern __shared__ __attribute__((aligned(16))) float lr_xs[];  // [C]
  constexpr int r = 4 * NR;
  const int t = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int id = ids[t];  // in flight while the row is staged (x is valid whatever the id)
  const int C4 = C / 4;
  float4* xs4 = (float4*)lr_xs;
  lr_stage<1>(x + (long long)t * (pro == LR_SWIGLU ? 2 * C : C), gain, xs4, 1, C, pro, eps);
  __syncthreads();
  if (id < 0 || id >= Rn) {  // uniform over the workgroup
    if (threadIdx.x < r) u[(long long)t * r + threadIdx.x] = 0.f;
    return;
  }
  const float* a0 = A + (long long)id * as;
  float acc[NR];
#pragma unroll
  for (int m = 0; m < NR; ++m) acc[m] = 0.f;
  for (int c = lane; c < C4; c += 64) {
    const float4 xv = xs4[c];
#pragma unroll
    for (int m = 0; m < NR; ++m) {
      const float4 av = ((const float4*)(a0 + (long long)(wv + 4 * m) * C))[c];
      float a = acc[m];
      a = fmaf(av.x, xv.x, a);
      a = fmaf(av.y, xv.y, a);
      a = fmaf(av.z, xv.z, a);
      a = fmaf(av.w, xv.w, a);
      acc[m] = a;
    }
  }
#pragma unroll
  for (int m = 0; m < NR; ++m) {
    const float s = wave_sum(acc[m]);
    if (lane == 0) u[(long long)t * r + wv + 4 * m] = s;
  }
}

// x [T][C] ([T][2C] for swiglu), A [Rn][r][C] with slots a_stride floats apart (0: one shared A),
// ids int32 [T], u [T][r]. r in {4, 8, 16}, 1 <= T <= 16, C % 4 == 0.
DDL_API int ddl_lora_rows_u(const float* x, const float* A, const int* ids, const float* gain, float* u, int T, int C,
                            int Rn, int r, long long a_stride, int pro, float eps, hipStream_t s) {
  if (!lin_rows_args_ok(x, A, gain, u, T, C, 1, pro)) return (int)hipErrorInvalidValue;
  if (!ids || Rn < 1 || !lr_rank_ok(r) || !lr_al16(x) || !lr_al16(A) || !lr_al16(u)) return (int)hipErrorInvalidValue;
  if (a_stride % 4 || (a_stride != 0 && a_stride < (long long)r * C)) return (int)hipErrorInvalidValue;
  const size_t lds = (size_t)C * sizeof(float);
  if (lds > (size_t)LR_LDS_BYTES) return (int)hipErrorInvalidValue;
#define LR_U(NR)                                                                                                  \
  hipLaunchKernelGGL(lora_rows_u_kernel<NR>, dim3(T), dim3(256), lds, s, x, A, ids, gain, u, C, Rn, a_stride, pro, eps)
  if (r == 4) LR_U(1);
  else if (r == 8) LR_U(2);
  else LR_U(4);
#undef LR_U
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Decode attention. qkv [B][3][H][HD] (one token), kc / vc [B][H][Smax][HD], lens [B], cos / sin
// [Smax][HD/2], o [B][H][HD], ws [B][H][NS][HD + 2] (NS > 1: m, l, unnormalised acc per split).
// Split sp covers cache rows [sp * chunk, min((sp + 1) * chunk, L)), chunk = ceil(Smax / NS); the
// new row (position L) comes from qkv and belongs to (split 0, wave 0, quad 0), which also stores
// it: no workgroup reads a row that another one writes in the same launch.
template <int HD>
__global__ __launch_bounds__(256) void attnf_decode_kernel(const float* __restrict__ qkv, float* __restrict__ kc,
                                                           float* __restrict__ vc, const int* __restrict__ lens,
                                                           const float* __restrict__ cosb,
                                                           const float* __restrict__ sinb, float* __restrict__ o,
                                                           float* __restrict__ ws, int H, int Smax, int NS,
                                                           int chunk, float sl2) {
  constexpr int DQ = HD / 4, REC = HD + 2;
  __shared__ float red[4][REC];
  const int h = blockIdx.x, b = blockIdx.y, sp = blockIdx.z;
  const int L = lens[b];
  if (L < 0 || L >= Smax) {  // frozen (uniform over the workgroup): zeros, nothing stored or read
    if (NS == 1 && threadIdx.x < HD) o[((long long)b * H + h) * HD + threadIdx.x] = 0.f;
    return;
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, g = lane & 3, qd = lane >> 2;
  const float* qp = qkv + ((long long)b * 3 * H + h) * HD + g * DQ;
  const float* cs = cosb + (long long)L * (HD / 2);
  const float* sn = sinb + (long long)L * (HD / 2);
  float qf[DQ], kf[DQ], vf[DQ], acc[DQ];
  dec_load<DQ>(qp, qf);
  dec_rope<DQ>(qf, cs, sn, g * DQ);
  dec_load<DQ>(qp + (long long)H * HD, kf);
  dec_rope<DQ>(kf, cs, sn, g * DQ);
  dec_load<DQ>(qp + 2LL * H * HD, vf);
  const float snew = dec_quad_sum(dec_dot<DQ>(qf, kf)) * sl2;
  const long long cbase = ((long long)b * H + h) * Smax * HD + g * DQ;
  const bool owner = sp == 0 && wv == 0 && qd == 0;
  float m = -INFINITY, l = 0.f;
#pragma unroll
  for (int d = 0; d < DQ; ++d) acc[d] = 0.f;
  if (owner) {
    dec_store<DQ>(kc + cbase + (long long)L * HD, kf);
    dec_store<DQ>(vc + cbase + (long long)L * HD, vf);
    m = snew;
    l = 1.f;
#pragma unroll
    for (int d = 0; d < DQ; ++d) acc[d] = vf[d];
  }
  const int j0 = sp * chunk, j1 = min(L, j0 + chunk);  // j1 <= L < Smax
  for (int j = j0 + wv * 16 + qd; j < j1; j += 64) {   // a quad's lanes share j
    dec_load<DQ>(kc + cbase + (long long)j * HD, kf);
    dec_load<DQ>(vc + cbase + (long long)j * HD, vf);
    const float sc = dec_quad_sum(dec_dot<DQ>(qf, kf)) * sl2;
    const float nm = fmaxf(m, sc);
    const float corr = exp2f(m - nm), p = exp2f(sc - nm);
    l = l * corr + p;
#pragma unroll
    for (int d = 0; d < DQ; ++d) acc[d] = acc[d] * corr + p * vf[d];
    m = nm;
  }
  // the wave's 16 quads: xor butterfly over the quad index
#pragma unroll
  for (int off = 4; off < 64; off <<= 1) {
    const float om = __shfl_xor(m, off), ol = __shfl_xor(l, off);
    const float nm = fmaxf(m, om);
    const float ca = dec_w(m, nm), cb = dec_w(om, nm);
    l = l * ca + ol * cb;
#pragma unroll
    for (int d = 0; d < DQ; ++d) acc[d] = acc[d] * ca + __shfl_xor(acc[d], off) * cb;
    m = nm;
  }
  if (qd == 0) {
    if (g == 0) {
      red[wv][0] = m;
      red[wv][1] = l;
    }
#pragma unroll
    for (int d = 0; d < DQ; ++d) red[wv][2 + g * DQ + d] = acc[d];
  }
  __syncthreads();
  if (threadIdx.x < HD) {  // the four waves in wave order
    const int d = threadIdx.x;
    float M = red[0][0];
#pragma unroll
    for (int k = 1; k < 4; ++k) M = fmaxf(M, red[k][0]);
    float Ls = 0.f, a = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float c = dec_w(red[k][0], M);
      Ls += red[k][1] * c;
      a += red[k][2 + d] * c;
    }
    if (NS == 1) {
      o[((long long)b * H + h) * HD + d] = a / Ls;  // Ls >= 1 term: the new row is always there
    } else {
      float* rec = ws + (((long long)b * H + h) * NS + sp) * REC;
      if (d == 0) {
        rec[0] = M;
        rec[1] = Ls;
      }
      rec[2 + d] = a;
    }
  }
}

// NS > 1: the splits' records in split order (split 0 is never empty: it holds the new row)
__global__ __launch_bounds__(128) void attnf_decode_merge_kernel(const float* __restrict__ ws,
                                                                 const int* __restrict__ lens,
                                                                 float* __restrict__ o, int H, int HD, int Smax,
                                                                 int NS) {
  const int h = blockIdx.x, b = blockIdx.y, d = threadIdx.x;
  if (d >= HD) return;
  const int L = lens[b];
  float* op = o + ((long long)b * H + h) * HD + d;
  if (L < 0 || L >= Smax) {
    *op = 0.f;
    return;
  }
  const int REC = HD + 2;
  const float* rec = ws + ((long long)b * H + h) * NS * REC;
  float M = rec[0];
  for (int s = 1; s < NS; ++s) M = fmaxf(M, rec[s * REC]);
  float Ls = 0.f, a = 0.f;
  for (int s = 0; s < NS; ++s) {
    const float c = dec_w(rec[s * REC], M);
    Ls += rec[s * REC + 1] * c;
    a += rec[s * REC + 2 + d] * c;
  }
  *op = a / Ls;
}

constexpr int DEC_MAX_SPLITS = 64;

DDL_API int ddl_attnf_decode(const float* qkv, float* kc, float* vc, const int* lens, const float* cosb,
                             const float* sinb, float* o, float* ws, int B, int H, int HD, int Smax, int NS,
                             float scale, hipStream_t s) {
  if (!qkv || !kc || !vc || !lens || !cosb || !sinb || !o) return (int)hipErrorInvalidValue;
  if (B < 1 || H < 1 || Smax < 1 || NS < 1 || NS > DEC_MAX_SPLITS || B > 65535 || (NS > 1 && !ws))
    return (int)hipErrorInvalidValue;
  const dim3 grid(H, B, NS);
  const int chunk = (Smax + NS - 1) / NS;
  const float sl2 = scale * DEC_LOG2E;
#define DEC_ATT(D)                                                                                              \
  hipLaunchKernelGGL(attnf_decode_kernel<D>, grid, dim3(256), 0, s, qkv, kc, vc, lens, cosb, sinb, o, ws, H, Smax, \
                     NS, chunk, sl2)
  switch (HD) {
    case 16: DEC_ATT(16); break;
    case 32: DEC_ATT(32); break;
    case 48: DEC_ATT(48); break;
    case 64: DEC_ATT(64); break;
    case 96: DEC_ATT(96); break;
    case 128: DEC_ATT(128); break;
    default: return (int)hipErrorInvalidValue;
  }
#undef DEC_ATT
  int rc = (int)hipGetLastError();
  if (rc || NS == 1) return rc;
  hipLaunchKernelGGL(attnf_decode_merge_kernel, dim3(H, B), dim3(128), 0, s, ws, lens, o, H, HD, Smax, NS);
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Prefill append: qkv [B][T][3][H][HD] -> cache rows pos0 + t (rows at or past Smax are dropped)
__global__ void kv_append_kernel(const float* __restrict__ qkv, float* __restrict__ kc, float* __restrict__ vc,
                                 const float* __restrict__ cosb, const float* __restrict__ sinb, int B, int T, int H,
                                 int HD, int Smax, int pos0) {
  const int D4 = HD / 4;
  const long long n = (long long)B * T * H * D4;
  GSTRIDE_LOOP(e, n) {
    const int d = (int)(e % D4) * 4;
    long long r = e / D4;
    const int h = (int)(r % H);
    r /= H;
    const int t = (int)(r % T), b = (int)(r / T);
    const int pos = pos0 + t;
    if (pos >= Smax) continue;
    const float* src = qkv + (((long long)b * T + t) * 3 + 1) * H * HD + (long long)h * HD + d;
    const float4 k = *(const float4*)src, v = *(const float4*)(src + (long long)H * HD);
    const float* cs = cosb + (long long)pos * (HD / 2) + d / 2;
    const float* sn = sinb + (long long)pos * (HD / 2) + d / 2;
    const long long at = (((long long)b * H + h) * Smax + pos) * HD + d;
    *(float4*)(kc + at) = make_float4(k.x * cs[0] - k.y * sn[0], k.x * sn[0] + k.y * cs[0],
                                      k.z * cs[1] - k.w * sn[1], k.z * sn[1] + k.w * cs[1]);
    *(float4*)(vc + at) = v;
  }
}

DDL_API int ddl_kv_append(const float* qkv, float* kc, float* vc, const float* cosb, const float* sinb, int B, int T,
                          int H, int HD, int Smax, int pos0, hipStream_t s) {
  if (!qkv || !kc || !vc || !cosb || !sinb || B < 1 || T < 1 || H < 1 || Smax < 1 || pos0 < 0)
    return (int)hipErrorInvalidValue;
  if (HD != 16 && HD != 32 && HD != 48 && HD != 64 && HD != 96 && HD != 128) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(kv_append_kernel, dim3(grid_for((long long)B * T * H * (HD / 4), 256)), dim3(256), 0, s, qkv, kc,
                     vc, cosb, sinb, B, T, H, HD, Smax, pos0);
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Sampler. One workgroup of 4 waves per row.
constexpr int SMP_E = 4, SMP_MAX_K = 1024;

// order-preserving key of a float (larger float <=> larger key; -0 counts as +0)
__device__ __forceinline__ uint32_t smp_key(float f) {
  const uint32_t u = __float_as_uint(f + 0.f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// inclusive prefix sum over the workgroup's 256 threads in thread order (sh: 4 ints)
__device__ __forceinline__ int smp_scan_incl(int v, int* sh) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int t = __shfl_up(v, off);
    if (lane >= off) v += t;
  }
  if (lane == 63) sh[wv] = v;
  __syncthreads();
  int add = 0;
  for (int k = 0; k < wv; ++k) add += sh[k];
  __syncthreads();
  return v + add;
}

struct SmpSel {  // the kept set: key > tau, or key == tau at an index <= cut
  uint32_t tau;
  int cut;
  float temp, zmax;  // weight = exp(logit / temp - zmax), zmax = max logit / temp
};

// Ordered running sum of the kept weights over [r0, r1) by one wave, starting from `carry`: lane l
// owns SMP_E consecutive elements of each 64 * SMP_E chunk, a shuffle scan orders the lanes, the
// chunks follow one another. `found` = lowest index whose running sum reaches `target` (else
// unchanged), `last` = highest kept index. Returns the running sum at r1 (the same bits in every lane).
__device__ __forceinline__ float smp_wave_cdf(const float* __restrict__ x, int r0, int r1, const SmpSel& sel,
                                              float carry, float target, int& found, int& last) {
  const int lane = threadIdx.x & 63;
  float run = carry;
  for (int base = r0; base < r1; base += 64 * SMP_E) {
    const int i0 = base + lane * SMP_E;
    float sfx[SMP_E], loc = 0.f;
    unsigned kept = 0;
#pragma unroll
    for (int e = 0; e < SMP_E; ++e) {
      const int i = i0 + e;
      float wt = 0.f;
      if (i < r1) {
        const float v = x[i];
        const uint32_t key = smp_key(v);
        if (key > sel.tau || (key == sel.tau && i <= sel.cut)) {
          wt = expf(v / sel.temp - sel.zmax);
          kept |= 1u << e;
        }
      }
      loc += wt;
      sfx[e] = loc;
    }
    float inc = loc;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const float t = __shfl_up(inc, off);
      if (lane >= off) inc += t;
    }
    float before = __shfl_up(inc, 1);
    if (lane == 0) before = 0.f;
    const float pre = run + before;
#pragma unroll
    for (int e = 0; e < SMP_E; ++e) {
      if (kept & (1u << e)) {
        last = i0 + e;
        if (found == INT_MAX && pre + sfx[e] >= target) found = i0 + e;
      }
    }
    run = run + __shfl(inc, 63);
  }
  return run;
}

__global__ __launch_bounds__(256) void sample_f32_kernel(const float* __restrict__ logits, int V, float temperature,
                                                         int top_k, uint2 seed, int eos_id, int Smax, int advance,
                                                         int* __restrict__ next_tok, int* __restrict__ out,
                                                         int out_cols, int* __restrict__ lens,
                                                         int* __restrict__ finished, int* __restrict__ step) {
  __shared__ int hist[256];
  __shared__ int shi[4], sh_digit, sh_krem, sh_cnt, sh_cut, sh_idx[4];
  __shared__ float shf[4];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const float* x = logits + (long long)b * V;
  const int st = step[b], fin = finished[b];
  int tok = 0;
  if (!fin) {  // uniform over the workgroup
    // ---- maximum, lowest index on ties
    float bm = -INFINITY;
    int bi = INT_MAX;
    for (int i = tid; i < V; i += 256) {
      const float v = x[i];
      if (v > bm || (v == bm && i < bi)) {
        bm = v;
        bi = i;
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float ov = __shfl_xor(bm, off);
      const int oi = __shfl_xor(bi, off);
      if (ov > bm || (ov == bm && oi < bi)) {
        bm = ov;
        bi = oi;
      }
    }
    if (lane == 0) {
      shf[wv] = bm;
      sh_idx[wv] = bi;
    }
    __syncthreads();
    bm = shf[0];
    bi = sh_idx[0];
#pragma unroll
    for (int k = 1; k < 4; ++k)
      if (shf[k] > bm || (shf[k] == bm && sh_idx[k] < bi)) {
        bm = shf[k];
        bi = sh_idx[k];
      }
    __syncthreads();
    tok = bi;
    if (temperature > 0.f) {
      SmpSel sel;
      sel.tau = 0u;  // every key >= 0: everything kept
      sel.cut = V;
      sel.temp = temperature;
      sel.zmax = bm / temperature;
      if (top_k > 0 && top_k < V) {
        // ---- exact threshold: 4 passes of 8 bits over the keys, most significant first
        uint32_t prefix = 0u;
        int krem = top_k, eqcnt = 0;
        for (int pass = 0; pass < 4; ++pass) {
          const int shift = 24 - 8 * pass;
          const uint32_t himask = pass == 0 ? 0u : (0xFFFFFFFFu << (shift + 8));
          hist[tid] = 0;
          __syncthreads();
          for (int i = tid; i < V; i += 256) {
            const uint32_t key = smp_key(x[i]);
            if ((key & himask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1);
          }
          __syncthreads();
          const int bin = 255 - tid, cnt = hist[bin];
          const int incl = smp_scan_incl(cnt, shi);  // keys of the prefix with digit >= bin
          if (incl >= krem && incl - cnt < krem) {   // exactly one thread
            sh_digit = bin;
            sh_krem = krem - (incl - cnt);
            sh_cnt = cnt;
          }
          __syncthreads();
          prefix |= (uint32_t)sh_digit << shift;
          krem = sh_krem;
          eqcnt = sh_cnt;
          __syncthreads();
        }
        sel.tau = prefix;
        if (krem < eqcnt) {
          // ---- more logits equal the threshold than fit: keep the krem lowest indices
          const int rw = (V + 3) / 4, r0 = min(V, wv * rw), r1 = min(V, r0 + rw);
          int c = 0;
          for (int i = r0 + lane; i < r1; i += 64) c += smp_key(x[i]) == sel.tau ? 1 : 0;
#pragma unroll
          for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
          if (lane == 0) shi[wv] = c;
          __syncthreads();
          int run = 0;
          for (int k = 0; k < wv; ++k) run += shi[k];
          for (int base = r0; base < r1; base += 64) {
            const int i = base + lane;
            const bool eq = i < r1 && smp_key(x[i]) == sel.tau;
            const unsigned long long bal = __ballot(eq);
            const int below = __popcll(bal & ((1ull << lane) - 1ull));
            if (eq && run + below + 1 == krem) sh_cut = i;  // exactly one lane of the workgroup
            run += __popcll(bal);
          }
          __syncthreads();
          sel.cut = sh_cut;
          __syncthreads();
        }
      }
      // ---- Z, then the inverse CDF in vocabulary order: wave w owns the w-th quarter of the row
      const int rw = (V + 3) / 4, r0 = min(V, wv * rw), r1 = min(V, r0 + rw);
      int found = INT_MAX, last = -1;
      const float tw = smp_wave_cdf(x, r0, r1, sel, 0.f, INFINITY, found, last);
      if (lane == 0) shf[wv] = tw;
      __syncthreads();
      float carry = 0.f, Z = 0.f;
      for (int k = 0; k < 4; ++k) {
        if (k == wv) carry = Z;
        Z += shf[k];
      }
      const float u = u32_to_unit(philox4x32(make_uint4((uint32_t)st, (uint32_t)b, 0u, 0u), seed).x);
      found = INT_MAX;
      last = -1;
      smp_wave_cdf(x, r0, r1, sel, carry, u * Z, found, last);
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        found = min(found, __shfl_xor(found, off));
        last = max(last, __shfl_xor(last, off));
      }
      __syncthreads();
      if (lane == 0) {
        shi[wv] = found;
        sh_idx[wv] = last;
      }
      __syncthreads();
      found = min(min(shi[0], shi[1]), min(shi[2], shi[3]));
      last = max(max(sh_idx[0], sh_idx[1]), max(sh_idx[2], sh_idx[3]));
      // rounding may leave the last running sum an ulp short of Z at u = 1: the last kept index
      tok = found != INT_MAX ? found : last;
    }
    if (tok < 0 || tok >= V) tok = 0;  // a row of NaNs: still a valid token
  } else {
    tok = eos_id;
  }
  if (tid == 0) {
    next_tok[b] = tok;
    if (out && st >= 0 && st < out_cols) out[(long long)b * out_cols + st] = tok;
    if (!fin) {
      const int L = lens[b];
      if (advance && L >= 0 && L < Smax) lens[b] = L + 1;
      if (eos_id >= 0 && tok == eos_id) finished[b] = 1;
    }
    step[b] = st + 1;
  }
}

// logits [B][V]; next_tok / lens / finished / step: int32 [B] (step[b] = the row's Philox counter and
// output column, every row advanced by its own workgroup); out int32 [B][out_cols] or null
DDL_API int ddl_sample_f32(const float* logits, int B, int V, float temperature, int top_k,
                           unsigned long long seed, int eos_id, int Smax, int advance, int* next_tok, int* out,
                           int out_cols, int* lens, int* finished, int* step, hipStream_t s) {
  if (!logits || !next_tok || !lens || !finished || !step || B < 1 || V < 1) return (int)hipErrorInvalidValue;
  if (!(temperature >= 0.f) || temperature > 3.0e38f || top_k < 0 || top_k > SMP_MAX_K || eos_id >= V ||
      out_cols < 0 || (out_cols > 0 && !out))
    return (int)hipErrorInvalidValue;
  const uint2 key = make_uint2((uint32_t)seed, (uint32_t)(seed >> 32));
  hipLaunchKernelGGL(sample_f32_kernel, dim3(B), dim3(256), 0, s, logits, V, temperature, top_k, key, eos_id, Smax,
                     advance, next_tok, out_cols > 0 ? out : nullptr, out_cols, lens, finished, step);
  return (int)hipGetLastError();
}
