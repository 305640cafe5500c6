// Secure aggregation (Bonawitz et al., CCS 2017) [north-star, absent in reference]: clients upload
// fixed-point updates hidden under pairwise one-time masks that cancel in the sum, plus a self mask
// each; the server sums the uploads mod 2^32, takes off the survivors' self masks and the pair masks
// the dropped clients left behind, and dequantises. Key agreement and secret sharing are simulated:
// every mask is a pure function of (seed, round, pair, coordinate).
//
//   encode : d = fl32(x - c) (no centre: x), p = fl32(cs * d), r = rint((double)p * 2^f), ties to
//            even; q = (int)r for |r| <= lim = (2^31 - 1) / n, +-lim beyond (counted in sat[g]),
//            0 for NaN (counted). A row with cs == 0 is not read: q = 0, not counted, still masked.
//   mask   : m(a, b, e), a <= b, is word e & 3 of philox4x32(counter (Q_lo, Q_hi, (a << 16) | b,
//            round), key (seed_lo ^ SECAGG_TAG, seed_hi)), Q = e >> 2. Client i of cohort U uploads
//            y = q + m(i, i, e) + sum_{j in U, j != i} s_ij m(min, max, e), s_ij = +1 for i < j, else -1.
//   open   : T = sum_rows y - sum_{i in S} m(i, i, e) - sum_{i in S, d in D} s_id m(min, max, e),
//            delta = (float)(int)T * 2^-f (the conversion rounds to nearest even).
//
//   ddl_secagg_mask : words [G][P], sat [G]; n Philox calls per quad per row, or (pair_shared, 2..8
//                     rows) one call for a pair of two local clients
//   ddl_secagg_sum  : out [P] = the wrap-around sum of R rows (a rank's partial)
//   ddl_secagg_open : delta [P] from R rows; ns + ns * nd Philox calls per quad
//
// Everything is integer arithmetic mod 2^32: any grouping of the adds gives the same bits, and
// n * lim < 2^31 keeps the opened sum from wrapping. All three run on quad_stream (quad_stream.h):
// 16-B accesses where every base is 16-B aligned and every row stride a multiple of 4, element by
// element otherwise (a whole Philox call for one word there), one body for both. No float atomics,
// no scratch; sat is folded with integer adds.
#include "quad_stream.h"

constexpr uint32_t SECAGG_TAG = 0x9b05688cu;
constexpr int SECAGG_MIN_BITS = 8, SECAGG_MAX_BITS = 30, SECAGG_MAX_CLIENTS = 65536;

// blocks along a row: about 2048 in all over the G rows, the rest by the grid-stride loop (the
// kernels are bound by the Philox rounds, not by memory: more blocks than fit at once buy nothing)
static int secagg_row_blocks(int G, long long P) {
  const int bx = grid_for((P + 3) / 4, 256);
  const int lim = G >= 2048 ? 1 : 2048 / (G < 1 ? 1 : G);
  return bx < lim ? bx : lim;
}

DDL_API int ddl_secagg_row_blocks(int G, long long P) { return (G < 1 || P < 1) ? 0 : secagg_row_blocks(G, P); }

// m(a, b, .) over the W coordinates from e on (W = 4: e is a multiple of 4, the whole call; W = 1:
// word e & 3 of the call of e's quad)
template <int W>
__device__ __forceinline__ uvec<W> pair_mask(uint2 key, long long e, uint32_t a, uint32_t b, uint32_t round) {
  const unsigned long long Q = (unsigned long long)e >> 2;
  const uint4 r = philox4x32(make_uint4((uint32_t)Q, (uint32_t)(Q >> 32), (a << 16) | b, round), key);
  uvec<W> m;
  if constexpr (W == 4) {
    m[0] = r.x; m[1] = r.y; m[2] = r.z; m[3] = r.w;
  } else {
    const int k = (int)(e & 3);
    m[0] = k == 0 ? r.x : k == 1 ? r.y : k == 2 ? r.z : r.w;
  }
  return m;
}

// acc += s_ij m(min(i, j), max(i, j), .) for j != i
template <int W>
__device__ __forceinline__ void add_pair(uvec<W>& acc, uint2 key, long long e, uint32_t i, uint32_t j, uint32_t round) {
  const bool up = i < j;
  const uvec<W> m = pair_mask<W>(key, e, up ? i : j, up ? j : i, round);
#pragma unroll
  for (int k = 0; k < W; ++k) acc[k] = up ? acc[k] + m[k] : acc[k] - m[k];
}

// q of W coordinates of one row into acc (a row of weight zero is not read: 0 * NaN would be NaN);
// `over` counts the coordinates that left +-lim or were NaN
template <int W>
__device__ __forceinline__ uvec<W> encode_row(const float* __restrict__ row, const float* __restrict__ c, float k,
                                              long long e, double scale, double lim, int& over) {
#pragma clang fp contract(off)
  uvec<W> acc = uzero<W>();
  if (k != 0.f) {
    const fvec<W> v = ldv<W>(row + e);
    const fvec<W> m = c ? ldv<W>(c + e) : fzero<W>();
#pragma unroll
    for (int i = 0; i < W; ++i) {
      const float d = c ? v[i] - m[i] : v[i];
      const float p = k * d;
      const double r = rint((double)p * scale);
      int q;
      if (r != r) { q = 0; ++over; }
      else if (r > lim) { q = (int)lim; ++over; }
      else if (r < -lim) { q = -(int)lim; ++over; }
      else q = (int)r;
      acc[i] = (uint32_t)q;
    }
  }
  return acc;
}

// the row's count into sat[g]: integer adds, any order the same sum
__device__ __forceinline__ void flush_sat(int over, int* sat) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) over += __shfl_xor(over, o, 64);
  if ((threadIdx.x & 63) == 0 && over) atomicAdd(sat, over);
}

// The plain form: each row on its own, n Philox calls per quad per row.
__global__ __launch_bounds__(256) void secagg_mask_kernel(const float* __restrict__ X, long long ld,
                                                          const float* __restrict__ c, const float* __restrict__ cs,
                                                          const int* __restrict__ slot_client, int G, long long P,
                                                          const int* __restrict__ cohort, int n, int frac_bits,
                                                          uint2 key, uint32_t round, uint32_t* __restrict__ words,
                                                          long long ldw, int* __restrict__ sat) {
  const bool vec = (ld % 4) == 0 && (ldw % 4) == 0 && (((uintptr_t)X | (uintptr_t)c | (uintptr_t)words) & 15) == 0;
  const double scale = (double)(1u << frac_bits), lim = (double)(0x7fffffff / n);
  for (int g = blockIdx.y; g < G; g += gridDim.y) {
    const float* row = X + (long long)g * ld;
    uint32_t* out = words + (long long)g * ldw;
    const float k = cs[g];
    const uint32_t me = (uint32_t)slot_client[g];
    int over = 0;
    quad_stream(P, vec, [&](long long e, auto w) {
      constexpr int W = decltype(w)::value;
      uvec<W> acc = encode_row<W>(row, c, k, e, scale, lim, over);
      const uvec<W> self = pair_mask<W>(key, e, me, me, round);
#pragma unroll
      for (int i = 0; i < W; ++i) acc[i] += self[i];
      for (int j = 0; j < n; ++j) {
        const uint32_t other = (uint32_t)cohort[j];
        if (other != me) add_pair<W>(acc, key, e, me, other, round);
      }
      stv<W>(out + e, acc);
    });
    flush_sat(over, sat + g);
  }
}

// The pair-shared form, for 2 <= G <= SECAGG_SHARED_ROWS local rows: a thread holds its quad of
// every row, and a pair (i, j) with both clients local costs one Philox call, added to one row
// and taken off the other: G + G (G - 1) / 2 + G (n - G) calls per quad instead of G n. The same
// integer sums regrouped, so the same bits. The row loops are unrolled over the compile-time bound
// with uniform guards, so the accumulators stay in registers (4 G of them).
constexpr int SECAGG_SHARED_ROWS = 8;

__global__ __launch_bounds__(256) void secagg_mask_shared_kernel(const float* __restrict__ X, long long ld,
                                                                 const float* __restrict__ c,
                                                                 const float* __restrict__ cs,
                                                                 const int* __restrict__ slot_client, int G, long long P,
                                                                 const int* __restrict__ cohort, int n, int frac_bits,
                                                                 uint2 key, uint32_t round, uint32_t* __restrict__ words,
                                                                 long long ldw, int* __restrict__ sat) {
  constexpr int R = SECAGG_SHARED_ROWS;
  const bool vec = (ld % 4) == 0 && (ldw % 4) == 0 && (((uintptr_t)X | (uintptr_t)c | (uintptr_t)words) & 15) == 0;
  const double scale = (double)(1u << frac_bits), lim = (double)(0x7fffffff / n);
  uint32_t id[R];
  float k[R];
  int over[R];
#pragma unroll
  for (int g = 0; g < R; ++g) {
    id[g] = g < G ? (uint32_t)slot_client[g] : 0u;
    k[g] = g < G ? cs[g] : 0.f;
    over[g] = 0;
  }
  quad_stream(P, vec, [&](long long e, auto w) {
    constexpr int W = decltype(w)::value;
    uvec<W> acc[R];
#pragma unroll
    for (int g = 0; g < R; ++g) {
      if (g < G) {
        acc[g] = encode_row<W>(X + g * ld, c, k[g], e, scale, lim, over[g]);
        const uvec<W> self = pair_mask<W>(key, e, id[g], id[g], round);
#pragma unroll
        for (int i = 0; i < W; ++i) acc[g][i] += self[i];
      }
    }
    // local pairs: one call for both rows
#pragma unroll
    for (int g = 0; g < R; ++g) {
#pragma unroll
      for (int h = g + 1; h < R; ++h) {
        if (h < G) {
          const bool up = id[g] < id[h];
          const uvec<W> m = pair_mask<W>(key, e, up ? id[g] : id[h], up ? id[h] : id[g], round);
#pragma unroll
          for (int i = 0; i < W; ++i) {
            acc[g][i] = up ? acc[g][i] + m[i] : acc[g][i] - m[i];
            acc[h][i] = up ? acc[h][i] - m[i] : acc[h][i] + m[i];
          }
        }
      }
    }
    // the cohort's other members: a call per row
    for (int j = 0; j < n; ++j) {
      const uint32_t other = (uint32_t)cohort[j];
      bool local = false;
#pragma unroll
      for (int g = 0; g < R; ++g) local |= g < G && id[g] == other;
      if (local) continue;
#pragma unroll
      for (int g = 0; g < R; ++g)
        if (g < G) add_pair<W>(acc[g], key, e, id[g], other, round);
    }
#pragma unroll
    for (int g = 0; g < R; ++g)
      if (g < G) stv<W>(words + g * ldw + e, acc[g]);
  });
#pragma unroll
  for (int g = 0; g < R; ++g)
    if (g < G) flush_sat(over[g], sat + g);
}

__global__ __launch_bounds__(256) void secagg_sum_kernel(const uint32_t* __restrict__ words, long long ldw, int R,
                                                         long long P, uint32_t* __restrict__ out) {
  const bool vec = (ldw % 4) == 0 && (((uintptr_t)words | (uintptr_t)out) & 15) == 0;
  quad_stream(P, vec, [&](long long e, auto w) {
    constexpr int W = decltype(w)::value;
    uvec<W> acc = uzero<W>();
    for (int r = 0; r < R; ++r) {
      const uvec<W> v = ldv<W>(words + r * ldw + e);
#pragma unroll
      for (int i = 0; i < W; ++i) acc[i] += v[i];
    }
    stv<W>(out + e, acc);
  });
}

__global__ __launch_bounds__(256) void secagg_open_kernel(const uint32_t* __restrict__ words, long long ldw, int R,
                                                          long long P, const int* __restrict__ survivors, int ns,
                                                          const int* __restrict__ dropped, int nd, float unit,
                                                          uint2 key, uint32_t round, float* __restrict__ delta) {
  const bool vec = (ldw % 4) == 0 && (((uintptr_t)words | (uintptr_t)delta) & 15) == 0;
  quad_stream(P, vec, [&](long long e, auto w) {
#pragma clang fp contract(off)
    constexpr int W = decltype(w)::value;
    uvec<W> acc = uzero<W>();
    for (int r = 0; r < R; ++r) {
      const uvec<W> v = ldv<W>(words + r * ldw + e);
#pragma unroll
      for (int i = 0; i < W; ++i) acc[i] += v[i];
    }
    // take off what the survivors added: the negated upload masks of add_pair
    uvec<W> masks = uzero<W>();
    for (int s = 0; s < ns; ++s) {
      const uint32_t me = (uint32_t)survivors[s];
      const uvec<W> self = pair_mask<W>(key, e, me, me, round);
#pragma unroll
      for (int i = 0; i < W; ++i) masks[i] += self[i];
      for (int d = 0; d < nd; ++d) add_pair<W>(masks, key, e, me, (uint32_t)dropped[d], round);
    }
    fvec<W> o;
#pragma unroll
    for (int i = 0; i < W; ++i) o[i] = (float)(int)(acc[i] - masks[i]) * unit;
    stv<W>(delta + e, o);
  });
}

static bool secagg_bits_ok(int frac_bits) { return frac_bits >= SECAGG_MIN_BITS && frac_bits <= SECAGG_MAX_BITS; }
static uint2 secagg_key(unsigned long long seed) {
  return make_uint2((uint32_t)seed ^ SECAGG_TAG, (uint32_t)(seed >> 32));
}

DDL_API int ddl_secagg_mask(const float* X, long long ld, const float* center, const float* cs,
                            const int* slot_client, int G, long long P, const int* cohort, int n, int frac_bits,
                            unsigned long long seed, unsigned int round, int* words, long long ldw, int* sat,
                            int pair_shared, hipStream_t s) {
  if (!X || !cs || !slot_client || !cohort || !words || !sat || G < 1 || P < 1 || ld < P || ldw < P ||
      !secagg_bits_ok(frac_bits) || n < 1 || n > SECAGG_MAX_CLIENTS)
    return (int)hipErrorInvalidValue;
  const hipError_t rc = hipMemsetAsync(sat, 0, sizeof(int) * (size_t)G, s);
  if (rc != hipSuccess) return (int)rc;
  const uint2 key = secagg_key(seed);
  if (pair_shared && G >= 2 && G <= SECAGG_SHARED_ROWS) {
    hipLaunchKernelGGL(secagg_mask_shared_kernel, dim3(secagg_row_blocks(1, P)), dim3(256), 0, s, X, ld, center, cs,
                       slot_client, G, P, cohort, n, frac_bits, key, (uint32_t)round, (uint32_t*)words, ldw, sat);
  } else {
    const int gy = G < 65535 ? G : 65535;
    hipLaunchKernelGGL(secagg_mask_kernel, dim3(secagg_row_blocks(G, P), gy), dim3(256), 0, s, X, ld, center, cs,
                       slot_client, G, P, cohort, n, frac_bits, key, (uint32_t)round, (uint32_t*)words, ldw, sat);
  }
  return (int)hipGetLastError();
}

DDL_API int ddl_secagg_sum(const int* words, long long ldw, int R, long long P, int* out, hipStream_t s) {
  if (!words || !out || R < 1 || P < 1 || ldw < P) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(secagg_sum_kernel, dim3(secagg_row_blocks(1, P)), dim3(256), 0, s, (const uint32_t*)words,
                     ldw, R, P, (uint32_t*)out);
  return (int)hipGetLastError();
}

DDL_API int ddl_secagg_open(const int* words, long long ldw, int R, long long P, const int* survivors, int ns,
                            const int* dropped, int nd, int frac_bits, unsigned long long seed, unsigned int round,
                            float* delta, hipStream_t s) {
  if (!words || !delta || !survivors || R < 1 || P < 1 || ldw < P || ns < 1 || nd < 0 || (nd > 0 && !dropped) ||
      (long long)ns + nd > SECAGG_MAX_CLIENTS || !secagg_bits_ok(frac_bits))
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(secagg_open_kernel, dim3(secagg_row_blocks(1, P)), dim3(256), 0, s, (const uint32_t*)words,
                     ldw, R, P, survivors, ns, dropped, nd, 1.0f / (float)(1u << frac_bits), secagg_key(seed),
                     (uint32_t)round, delta);
  return (int)hipGetLastError();
}
