// The streaming skeleton of the fp32 federated kernels (aggregate.hip, clip_agg.hip, fedopt.hip,
// scaffold.hip): a grid-stride loop over quads of floats that hands each kernel's body either one
// whole quad (W = 4: one 16-byte access per operand) or one element at a time (W = 1: the tail, or
// every element when some base or row stride is not 16-B aligned). The body is written once, generic
// over W, so both paths run the same operations in the same order and give the same bits.
//
//   quad_stream(n, aligned, [&](long long e, auto w) {
//   #pragma clang fp contract(off)           // a lambda body is a function of its own: the
//     constexpr int W = decltype(w)::value;  // enclosing kernel's pragma does not reach into it
//     fvec<W> v = ldv<W>(src + e); ... stv<W>(dst + e, v);
//   });
#pragma once
#include "ddl_common.h"

template <int W> struct quad_width { static constexpr int value = W; };

// W floats in registers
template <int W> struct fvec {
  float v[W];
  __device__ __forceinline__ float& operator[](int i) { return v[i]; }
  __device__ __forceinline__ const float& operator[](int i) const { return v[i]; }
};

template <int W> __device__ __forceinline__ fvec<W> fzero() {
  fvec<W> r;
#pragma unroll
  for (int i = 0; i < W; ++i) r.v[i] = 0.f;
  return r;
}

template <int W> __device__ __forceinline__ fvec<W> ldv(const float* p) {
  static_assert(W == 1 || W == 4, "one element or one 16-byte quad");
  fvec<W> r;
  if constexpr (W == 4) {
    const float4 t = *(const float4*)p;
    r.v[0] = t.x; r.v[1] = t.y; r.v[2] = t.z; r.v[3] = t.w;
  } else {
    r.v[0] = *p;
  }
  return r;
}

template <int W> __device__ __forceinline__ void stv(float* p, const fvec<W>& x) {
  if constexpr (W == 4) *(float4*)p = make_float4(x.v[0], x.v[1], x.v[2], x.v[3]);
  else *p = x.v[0];
}

// W 32-bit words in registers: the integer rows of secagg.hip (sums mod 2^32)
template <int W> struct uvec {
  uint32_t v[W];
  __device__ __forceinline__ uint32_t& operator[](int i) { return v[i]; }
  __device__ __forceinline__ const uint32_t& operator[](int i) const { return v[i]; }
};

template <int W> __device__ __forceinline__ uvec<W> uzero() {
  uvec<W> r;
#pragma unroll
  for (int i = 0; i < W; ++i) r.v[i] = 0u;
  return r;
}

template <int W> __device__ __forceinline__ uvec<W> ldv(const uint32_t* p) {
  static_assert(W == 1 || W == 4, "one element or one 16-byte quad");
  uvec<W> r;
  if constexpr (W == 4) {
    const uint4 t = *(const uint4*)p;
    r.v[0] = t.x; r.v[1] = t.y; r.v[2] = t.z; r.v[3] = t.w;
  } else {
    r.v[0] = *p;
  }
  return r;
}

template <int W> __device__ __forceinline__ void stv(uint32_t* p, const uvec<W>& x) {
  if constexpr (W == 4) *(uint4*)p = make_uint4(x.v[0], x.v[1], x.v[2], x.v[3]);
  else *p = x.v[0];
}

// the bf16 image of x (W = 4: one 8-byte store)
template <int W> __device__ __forceinline__ void stv_bf16(bf16_t* p, const fvec<W>& x) {
  if constexpr (W == 4) {
    i2v o;
    o[0] = (int)pack_bf2(x.v[0], x.v[1]);
    o[1] = (int)pack_bf2(x.v[2], x.v[3]);
    *(i2v*)p = o;
  } else {
    *p = f2bf(x.v[0]);
  }
}

// acc += sum_g coeff[g] * src[g][e .. e + W), rows in order. Every product rounded on its own, then
// added: hipcc contracts a * b + c into an fma by default (also through __fmul_rn / __fadd_rn, whose
// header bodies carry the contract flag), which made the G-row single-process sum differ from
// per-rank partials summed across ranks. Without it: the same bits as clients spread over ranks
// (each rank's product, then the all-reduce add) for 2 ranks, and the reference's sum of
// n_k/n-scaled state dicts (hfl_complete.py:370-378).
template <int W>
__device__ __forceinline__ void add_weighted_rows(fvec<W>& acc, const float* __restrict__ src, long long ld,
                                                  const float* __restrict__ coeff, int G, long long e) {
#pragma clang fp contract(off)
  for (int g = 0; g < G; ++g) {
    const float c = coeff[g];
    const fvec<W> v = ldv<W>(src + g * ld + e);
#pragma unroll
    for (int i = 0; i < W; ++i) acc[i] = acc[i] + c * v[i];
  }
}

// body(e, quad_width<4>) for every whole quad [e, e + 4) of [0, n) when `aligned` (the caller's
// statement that e % 4 == 0 makes every operand address 16-B aligned); body(k, quad_width<1>) for
// every other element. The grid is 1-D in x: grid_for((n + 3) / 4, block).
template <class Body>
__device__ __forceinline__ void quad_stream(long long n, bool aligned, Body&& body) {
  // the launch's block size as a kernel reads blockDim.x (one scalar load): outside a __global__
  // function blockDim.x compiles to the general form, which allows for a partial last block and
  // puts a dependent vector load in front of the loop
  const long long block = __builtin_amdgcn_workgroup_size_x();
  for (long long t = blockIdx.x * block + threadIdx.x; t * 4 < n; t += gridDim.x * block) {
    const long long e = t * 4;
    if (e + 4 <= n && aligned) {
      body(e, quad_width<4>{});
    } else {
      for (long long k = e; k < min(n, e + 4); ++k) body(k, quad_width<1>{});
    }
  }
}
