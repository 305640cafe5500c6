// Compressed client uploads with error feedback (Stich et al. 2018; Karimireddy et al. 2019)
// [north-star, absent in reference]: slot g's trained row y_g is rewritten in place to what the
// server would decode, x + q(u), u = (y_g - x) + e_i, where e_i is row slot_client[g] of an error
// bank [N][ld] that takes what the codec dropped (no bank: u = y_g - x, the dropped part is lost).
// A NaN / Inf u_j is passed through: row entry x_j + u_j, bank entry untouched, and it takes no part
// in selection, scale or counts.
//
//   ddl_topk_compress     : keep the entries with |u_j| >= tau_g, tau_g the k-th largest finite
//                           non-zero magnitude of the row (the smallest when there are fewer),
//                           magnitudes compared as the integer bits of |u_j|, every tie kept.
//                           An exact radix select on the 31 magnitude bits, digits 11 + 10 + 10:
//                             form   : row <- u, histogram of bits 30..20       4P floats per row
//                             digit  : histogram of the next 10 bits of the
//                                      entries under the chosen prefix, twice   1P each
//                             apply  : row <- x + u or x, bank <- 0 or u        4P
//                           u lives in the row itself between the passes (the row is rewritten
//                           anyway), so there is no [G][P] workspace with or without a bank. The
//                           histograms are integer: LDS counts per workgroup, flushed with integer
//                           adds into the row's global bins; a one-block launch per row picks the
//                           digit after each histogram. nnz_g comes out of the counts (entries
//                           above tau + the bin of tau), not out of the apply pass.
//   ddl_quantize_compress : QSGD-style stochastic levels per bucket of 256 columns, one pass, 5P:
//                           a wave owns a bucket (64 lanes x one quad), the scale s is the wave's
//                           integer max of the finite magnitude bits, a = (|u| / s) * L,
//                           l = min(L, floor(a) + (frac(a) >= r)), q = sign(u) * s * (l / L),
//                           row <- x + q, bank <- u - q. r = u32_to_unit of word j & 3 of
//                           philox4x32(counter (j >> 2, client, TAG, round), key seed): a pure
//                           function of (seed, round, client, column).
//
// The streaming passes run on quad_stream (quad_stream.h): 16-B accesses where every base is 16-B
// aligned and every row stride a multiple of 4 floats, element by element otherwise, one body for
// both. Every add, subtract, multiply and divide is rounded on its own (no contraction); no float
// atomics, and no result depends on the order in which workgroups arrive.
#include "quad_stream.h"

constexpr uint32_t EXP_MASK = 0x7f800000u;  // magnitude bits >= this: Inf / NaN
constexpr int TOPK_BINS0 = 2048, TOPK_BINS = 1024;
// uint32 per row: the three histograms, then {prefix, rank left, entries above, tau}
constexpr int TOPK_STATE = TOPK_BINS0 + 2 * TOPK_BINS;
constexpr int TOPK_WS_ROW = TOPK_STATE + 4;
constexpr uint32_t QUANT_TAG = 0x510e527fu;

// blocks along a row: about 2048 in all over the G rows, as the squared norms of clip_agg.hip (the
// histogram passes end in a barrier and a flush of their bins, so few long blocks beat many short)
static int compress_row_blocks(int G, long long P) {
  const int bx = grid_for((P + 3) / 4, 256);
  const int lim = G >= 2048 ? 1 : 2048 / (G < 1 ? 1 : G);
  return bx < lim ? bx : lim;
}

DDL_API int ddl_compress_row_blocks(int G, long long P) { return (G < 1 || P < 1) ? 0 : compress_row_blocks(G, P); }
DDL_API long long ddl_topk_workspace(int G) { return G < 1 ? 0 : (long long)G * TOPK_WS_ROW; }

__device__ __forceinline__ uint32_t mag_bits(float u) { return __float_as_uint(u) & 0x7fffffffu; }
// a magnitude that takes part in the selection: finite and not zero
__device__ __forceinline__ bool mag_counts(uint32_t key) { return key != 0u && key < EXP_MASK; }

// the block's LDS bins -> the row's global bins (integer adds: any order, the same sums)
template <int BINS> __device__ __forceinline__ void flush_bins(uint32_t* lds, uint32_t* glob) {
  __syncthreads();
  for (int b = threadIdx.x; b < BINS; b += 256) {
    const uint32_t c = lds[b];
    if (c) atomicAdd(glob + b, c);
    lds[b] = 0;
  }
  __syncthreads();
}

// rows alias nothing but themselves; a slot's bank row is read here and written by the apply pass
__global__ __launch_bounds__(256) void topk_form_kernel(float* rows, long long ldy, const float* __restrict__ x,
                                                        const float* __restrict__ bank, long long ld,
                                                        const int* __restrict__ slot_client, int G, long long P,
                                                        uint32_t* ws) {
  __shared__ uint32_t bins[TOPK_BINS0];
  for (int b = threadIdx.x; b < TOPK_BINS0; b += 256) bins[b] = 0;
  __syncthreads();
  for (int g = blockIdx.y; g < G; g += gridDim.y) {
    float* row = rows + (long long)g * ldy;
    const float* e_row = bank ? bank + (long long)slot_client[g] * ld : nullptr;
    const bool vec = (ldy % 4) == 0 && (!bank || (ld % 4) == 0) && (((uintptr_t)rows | (uintptr_t)x | (uintptr_t)bank) & 15) == 0;
    quad_stream(P, vec, [&](long long e, auto w) {
#pragma clang fp contract(off)
      constexpr int W = decltype(w)::value;
      const fvec<W> yv = ldv<W>(row + e), xv = ldv<W>(x + e);
      fvec<W> u;
      if (e_row) {
        const fvec<W> ev = ldv<W>(e_row + e);
#pragma unroll
        for (int i = 0; i < W; ++i) u[i] = (yv[i] - xv[i]) + ev[i];
      } else {
#pragma unroll
        for (int i = 0; i < W; ++i) u[i] = yv[i] - xv[i];
      }
      stv<W>(row + e, u);
#pragma unroll
      for (int i = 0; i < W; ++i) {
        const uint32_t key = mag_bits(u[i]);
        if (mag_counts(key)) atomicAdd(&bins[key >> 20], 1u);
      }
    });
    flush_bins<TOPK_BINS0>(bins, ws + (long long)g * TOPK_WS_ROW);
  }
}

// level 1: bits 19..10 of the entries whose bits 30..20 are the prefix; level 2: bits 9..0 of the
// entries whose bits 30..10 are the prefix. Reads the row (it holds u) only.
__global__ __launch_bounds__(256) void topk_digit_kernel(const float* __restrict__ rows, long long ldy, int G,
                                                         long long P, uint32_t* ws, int level) {
  __shared__ uint32_t bins[TOPK_BINS];
  for (int b = threadIdx.x; b < TOPK_BINS; b += 256) bins[b] = 0;
  __syncthreads();
  const int shift = level == 1 ? 10 : 0;
  for (int g = blockIdx.y; g < G; g += gridDim.y) {
    const float* row = rows + (long long)g * ldy;
    uint32_t* wr = ws + (long long)g * TOPK_WS_ROW;
    const uint32_t prefix = wr[TOPK_STATE];
    const bool vec = (ldy % 4) == 0 && ((uintptr_t)rows & 15) == 0;
    quad_stream(P, vec, [&](long long e, auto w) {
      constexpr int W = decltype(w)::value;
      const fvec<W> u = ldv<W>(row + e);
#pragma unroll
      for (int i = 0; i < W; ++i) {
        const uint32_t key = mag_bits(u[i]);
        if (mag_counts(key) && (key >> (shift + 10)) == prefix) atomicAdd(&bins[(key >> shift) & 1023u], 1u);
      }
    });
    flush_bins<TOPK_BINS>(bins, wr + TOPK_BINS0 + (level - 1) * TOPK_BINS);
  }
}

// One block per row picks the digit of tau in the histogram of `level`: the bin b, from the top,
// at which the count of entries reaches the rank still wanted. Level 0 also bounds the rank by the
// number of entries that count (fewer than k: tau is the smallest), and an empty row gets a tau no
// finite magnitude reaches. The last level writes tau and nnz = entries above tau + entries at tau.
__global__ __launch_bounds__(256) void topk_pick_kernel(uint32_t* ws, int G, unsigned long long k, int level,
                                                        int* __restrict__ nnz) {
  __shared__ uint32_t part[256];
  const int nb = level == 0 ? TOPK_BINS0 : TOPK_BINS;
  const int per = nb / 256;
  for (int g = blockIdx.x; g < G; g += gridDim.x) {
    uint32_t* wr = ws + (long long)g * TOPK_WS_ROW;
    const uint32_t* h = wr + (level == 0 ? 0 : TOPK_BINS0 + (level - 1) * TOPK_BINS);
    uint32_t* state = wr + TOPK_STATE;
    uint32_t s = 0;
    for (int j = 0; j < per; ++j) s += h[threadIdx.x * per + j];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t t = 0;
      for (int i = 0; i < 256; ++i) t += part[i];
      uint32_t prefix = level == 0 ? 0u : state[0];
      uint32_t want = level == 0 ? (uint32_t)(k < (unsigned long long)t ? k : t) : state[1];
      uint32_t above = level == 0 ? 0u : state[2];
      if (t == 0) {  // nothing counts in this row: nothing is kept
        state[0] = 0xffffffffu; state[1] = 0; state[2] = 0; state[3] = EXP_MASK;
        if (level == 2) nnz[g] = 0;
      } else {
        // want >= 1 and want <= t: the walk ends inside the histogram
        uint32_t cum = 0;
        int c = 255;
        while (cum + part[c] < want) cum += part[c--];
        int b = c * per + per - 1;
        while (cum + h[b] < want) cum += h[b--];
        prefix = (prefix << (level == 0 ? 11 : 10)) | (uint32_t)b;
        state[0] = prefix;
        state[1] = want - cum;
        state[2] = above + cum;
        if (level == 2) {
          state[3] = prefix;
          nnz[g] = (int)(above + cum + h[b]);
        }
      }
    }
    __syncthreads();
  }
}

// row <- x + u (kept, or passed through) or the bits of x (dropped); bank <- +0 (kept) or u
// (dropped), a passed-through entry keeps its bank bits
__global__ __launch_bounds__(256) void topk_apply_kernel(float* rows, long long ldy, const float* __restrict__ x,
                                                         float* bank, long long ld,
                                                         const int* __restrict__ slot_client, int G, long long P,
                                                         const uint32_t* __restrict__ ws) {
  for (int g = blockIdx.y; g < G; g += gridDim.y) {
    float* row = rows + (long long)g * ldy;
    float* e_row = bank ? bank + (long long)slot_client[g] * ld : nullptr;
    const uint32_t tau = ws[(long long)g * TOPK_WS_ROW + TOPK_STATE + 3];
    const bool vec = (ldy % 4) == 0 && (!bank || (ld % 4) == 0) && (((uintptr_t)rows | (uintptr_t)x | (uintptr_t)bank) & 15) == 0;
    quad_stream(P, vec, [&](long long e, auto w) {
#pragma clang fp contract(off)
      constexpr int W = decltype(w)::value;
      const fvec<W> u = ldv<W>(row + e), xv = ldv<W>(x + e);
      fvec<W> o, b;
      bool through = false;
#pragma unroll
      for (int i = 0; i < W; ++i) {
        const uint32_t key = mag_bits(u[i]);
        const bool nonfinite = key >= EXP_MASK;
        const bool keep = mag_counts(key) && key >= tau;
        o[i] = (keep || nonfinite) ? xv[i] + u[i] : xv[i];
        b[i] = keep ? 0.f : u[i];
        through |= nonfinite;
      }
      stv<W>(row + e, o);
      if (e_row) {
        if (!through) {
          stv<W>(e_row + e, b);
        } else {
#pragma unroll
          for (int i = 0; i < W; ++i)
            if (mag_bits(u[i]) < EXP_MASK) e_row[e + i] = b[i];
        }
      }
    });
  }
}

DDL_API int ddl_topk_compress(float* rows, long long ldy, const float* x, float* bank, long long ld,
                              const int* slot_client, int G, long long P, long long k, int* nnz, unsigned int* ws,
                              long long ws_cap, hipStream_t s) {
  if (G < 1 || P < 1 || k < 1 || !rows || !x || !nnz || !ws || ws_cap < ddl_topk_workspace(G) || (G > 1 && ldy < P) ||
      (bank && (!slot_client || ld < P)))
    return (int)hipErrorInvalidValue;
  const hipError_t rc = hipMemsetAsync(ws, 0, sizeof(uint32_t) * (size_t)ddl_topk_workspace(G), s);
  if (rc != hipSuccess) return (int)rc;
  const int gy = G < 65535 ? G : 65535;
  const dim3 grid(compress_row_blocks(G, P), gy), pick(gy < 1024 ? gy : 1024);
  hipLaunchKernelGGL(topk_form_kernel, grid, dim3(256), 0, s, rows, ldy, x, bank, ld, slot_client, G, P, ws);
  hipLaunchKernelGGL(topk_pick_kernel, pick, dim3(256), 0, s, ws, G, (unsigned long long)k, 0, nnz);
  for (int level = 1; level <= 2; ++level) {
    hipLaunchKernelGGL(topk_digit_kernel, grid, dim3(256), 0, s, rows, ldy, G, P, ws, level);
    hipLaunchKernelGGL(topk_pick_kernel, pick, dim3(256), 0, s, ws, G, (unsigned long long)k, level, nnz);
  }
  hipLaunchKernelGGL(topk_apply_kernel, grid, dim3(256), 0, s, rows, ldy, x, bank, ld, slot_client, G, P, ws);
  return (int)hipGetLastError();
}

// One quad of one bucket. The loop runs whole waves (every lane of a wave that owns a bucket takes
// part in the scale's reduction; lanes past the row hold no element), so it keeps a loop of its
// own next to quad_stream: thread t owns columns [4t, 4t + 4), wave t >> 6 the bucket of that index.
__global__ __launch_bounds__(256) void quantize_kernel(float* rows, long long ldy, const float* __restrict__ x,
                                                       float* bank, long long ld, const int* __restrict__ slot_client,
                                                       int G, long long P, int L, uint2 key, uint32_t round,
                                                       signed char* __restrict__ levels, float* __restrict__ scales) {
#pragma clang fp contract(off)
  const long long nq = (P + 3) / 4, nq_waves = (nq + 63) & ~63LL, nb = (P + 255) / 256;
  const float fL = (float)L;
  for (int g = blockIdx.y; g < G; g += gridDim.y) {
    float* row = rows + (long long)g * ldy;
    const uint32_t client = (uint32_t)slot_client[g];
    float* e_row = bank ? bank + (long long)client * ld : nullptr;
    const bool vec = (ldy % 4) == 0 && (!bank || (ld % 4) == 0) && (((uintptr_t)rows | (uintptr_t)x | (uintptr_t)bank) & 15) == 0;
    for (long long t = blockIdx.x * 256LL + threadIdx.x; t < nq_waves; t += gridDim.x * 256LL) {
      const long long e = t * 4;
      const int cnt = e + 4 <= P ? 4 : (e < P ? (int)(P - e) : 0);
      float u[4] = {0.f, 0.f, 0.f, 0.f}, xv[4] = {0.f, 0.f, 0.f, 0.f};
      if (cnt == 4 && vec) {
        const fvec<4> a = ldv<4>(row + e), c = ldv<4>(x + e);
        const fvec<4> b = e_row ? ldv<4>(e_row + e) : fzero<4>();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          xv[i] = c[i];
          u[i] = e_row ? (a[i] - c[i]) + b[i] : a[i] - c[i];
        }
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          if (i < cnt) {
            xv[i] = x[e + i];
            u[i] = e_row ? (row[e + i] - xv[i]) + e_row[e + i] : row[e + i] - xv[i];
          }
        }
      }
      // the bucket's scale: the largest finite magnitude, as integer bits (exact)
      uint32_t m = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const uint32_t kb = mag_bits(u[i]);
        if (i < cnt && kb < EXP_MASK && kb > m) m = kb;
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const uint32_t other = (uint32_t)__shfl_xor((int)m, o, 64);
        m = other > m ? other : m;
      }
      if (cnt == 0) continue;
      const float sc = __uint_as_float(m);
      if (scales && (threadIdx.x & 63) == 0) scales[(long long)g * nb + (t >> 6)] = sc;
      uint32_t r[4] = {0u, 0u, 0u, 0u};
      if (m != 0u) {
        const uint4 p = philox4x32(make_uint4((uint32_t)t, client, QUANT_TAG, round), key);
        r[0] = p.x; r[1] = p.y; r[2] = p.z; r[3] = p.w;
      }
      float o[4], b[4];
      int lv[4];
      bool through = false;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const uint32_t kb = mag_bits(u[i]);
        const bool nonfinite = kb >= EXP_MASK;
        float q = 0.f;
        int l = 0;
        if (!nonfinite && m != 0u) {
          const float a = (__uint_as_float(kb) / sc) * fL;
          const float fl = floorf(a);
          l = (int)fl + ((a - fl) >= u32_to_unit(r[i]) ? 1 : 0);
          l = l < L ? l : L;
          q = sc * ((float)l / fL);
          if (__float_as_uint(u[i]) >> 31) { q = -q; l = -l; }
        }
        lv[i] = l;
        o[i] = nonfinite ? xv[i] + u[i] : xv[i] + q;
        b[i] = u[i] - q;
        through |= nonfinite;
      }
      if (cnt == 4 && vec) {
        fvec<4> ov, bv;
#pragma unroll
        for (int i = 0; i < 4; ++i) { ov[i] = o[i]; bv[i] = b[i]; }
        stv<4>(row + e, ov);
        if (e_row && !through) stv<4>(e_row + e, bv);
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (i < cnt) row[e + i] = o[i];
      }
      if (e_row && !(cnt == 4 && vec && !through)) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (i < cnt && mag_bits(u[i]) < EXP_MASK) e_row[e + i] = b[i];
      }
      if (levels) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (i < cnt) levels[(long long)g * P + e + i] = (signed char)lv[i];
      }
    }
  }
}

DDL_API int ddl_quantize_compress(float* rows, long long ldy, const float* x, float* bank, long long ld,
                                  const int* slot_client, int G, long long P, int bits, unsigned long long seed,
                                  unsigned int round, signed char* levels, float* scales, hipStream_t s) {
  if (G < 1 || P < 1 || bits < 2 || bits > 8 || !rows || !x || !slot_client || (G > 1 && ldy < P) ||
      (bank && ld < P) || (P + 3) / 4 > 0xffffffffLL)
    return (int)hipErrorInvalidValue;
  const int gy = G < 65535 ? G : 65535;
  hipLaunchKernelGGL(quantize_kernel, dim3(compress_row_blocks(G, P), gy), dim3(256), 0, s, rows, ldy, x, bank, ld,
                     slot_client, G, P, (1 << (bits - 1)) - 1, make_uint2((uint32_t)seed, (uint32_t)(seed >> 32)),
                     (uint32_t)round, levels, scales);
  return (int)hipGetLastError();
}
