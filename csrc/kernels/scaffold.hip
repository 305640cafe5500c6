// SCAFFOLD (Karimireddy et al. 2020, Algorithm 1, option II) [north-star, absent in reference]: the
// round-end update of the control variates. The server holds c [P], client i holds row i of a bank
// [N][ld]; slot g of this GPU trained client slot_client[g] (an int32 table in device memory). The
// bank is read and written in place, never gathered into slot order. The control-variate local step
// is the SGD_CONTROL instance of ddl_sgd_corrected (fedopt.hip).
//
//   ddl_scaffold_finish : one thread owns a column quad, reads x[col], c[col] once, and walks the slots
//                         from 0 upward with acc = 0:
//                           t     = (x[col] - y[g][col]) * inv_klr[g]
//                           delta = t - c[col]
//                           bank[slot_client[g]][col] = bank[slot_client[g]][col] + delta
//                           acc   = acc + delta * inv_n
//                         a NaN / Inf delta leaves that bank entry as it was and adds nothing;
//                         dc[col] = acc, and with apply_c also c[col] = c[col] + acc (the c loaded
//                         before the loop). The slots' rows must be distinct bank rows (the host
//                         validates the table where it builds it). (3G + 3) P floats moved: y, bank
//                         read, bank write per slot; x, c read, dc written (+ P with apply_c).
//
// It streams on quad_stream (quad_stream.h): grid-stride, 256 threads, 16-B accesses where every base
// pointer is 16-B aligned and every row stride a multiple of 4 floats, element by element otherwise,
// one body for both; every add, subtract and multiply rounded on its own (no contraction), no LDS,
// no atomics, no scratch.
#include "quad_stream.h"

// One coordinate of one slot; a NaN / Inf delta leaves the bank entry b and acc untouched.
__device__ __forceinline__ void finish_update(float x, float y, float k, float c, float inv_n, float& b, float& acc) {
#pragma clang fp contract(off)
  const float t = (x - y) * k;
  const float delta = t - c;
  if ((__float_as_uint(delta) & 0x7f800000u) == 0x7f800000u) return;
  b = b + delta;
  acc = acc + delta * inv_n;
}

// x and dc alias nothing else; the rows y alias no bank row; c is read before it is written by the
// same thread
__global__ __launch_bounds__(256) void scaffold_finish_kernel(const float* __restrict__ y, long long ldy,
                                                              const float* __restrict__ x, float* c, float* bank,
                                                              long long ld, const int* __restrict__ slot_client,
                                                              const float* __restrict__ inv_klr, int G, float inv_n,
                                                              float* dc, long long P, int apply_c) {
  const bool vec = (ldy % 4) == 0 && (ld % 4) == 0 &&
                   (((uintptr_t)y | (uintptr_t)x | (uintptr_t)c | (uintptr_t)bank | (uintptr_t)dc) & 15) == 0;
  quad_stream(P, vec, [&](long long e, auto w) {
#pragma clang fp contract(off)
    constexpr int W = decltype(w)::value;
    const fvec<W> xv = ldv<W>(x + e), cv = ldv<W>(c + e);
    fvec<W> acc = fzero<W>();
    // four slots at a time: their loads are issued before the first bank store (the slots' bank
    // rows are distinct), the updates then run in slot order
    for (int g0 = 0; g0 < G; g0 += 4) {
      fvec<W> yv[4], bv[4];
      float k[4];
      float* bp[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (g0 + j < G) {
          bp[j] = bank + (long long)slot_client[g0 + j] * ld + e;
          yv[j] = ldv<W>(y + (g0 + j) * ldy + e);
          bv[j] = ldv<W>(bp[j]);
          k[j] = inv_klr[g0 + j];
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (g0 + j < G) {
          // a skipped coordinate stores back the bits it loaded
#pragma unroll
          for (int i = 0; i < W; ++i) finish_update(xv[i], yv[j][i], k[j], cv[i], inv_n, bv[j][i], acc[i]);
          stv<W>(bp[j], bv[j]);
        }
      }
    }
    stv<W>(dc + e, acc);
    if (apply_c) {
      fvec<W> o;
#pragma unroll
      for (int i = 0; i < W; ++i) o[i] = cv[i] + acc[i];
      stv<W>(c + e, o);
    }
  });
}

DDL_API int ddl_scaffold_finish(const float* y, long long ldy, const float* x, float* c, float* bank, long long ld,
                                const int* slot_client, const float* inv_klr, int G, float inv_n, float* dc,
                                long long P, int apply_c, hipStream_t s) {
  if (G < 1 || P < 1 || !y || !x || !c || !bank || !slot_client || !inv_klr || !dc || ld < P || (G > 1 && ldy < P))
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(scaffold_finish_kernel, dim3(grid_for((P + 3) / 4, 256)), dim3(256), 0, s, y, ldy, x, c, bank,
                     ld, slot_client, inv_klr, G, inv_n, dc, P, apply_c);
  return (int)hipGetLastError();
}
