// SCAFFOLD (Karimireddy et al. 2020, Algorithm 1, option II) [north-star, absent in reference]: the
// control-variate local step and the round-end update of the control variates. The server holds
// c [P], client i holds row i of a bank [N][ld]; slot g of this GPU trains client slot_client[g]
// (an int32 table in device memory, so a captured round graph keeps its pointers and the next
// round only overwrites the table's contents). The bank is read and written in place, never
// gathered into slot order.
//
//   ddl_sgd_scaffold    : rows p/g/mom/shadow [G][P]:
//                           d = g * grad_scale + wd * p
//                           d = d + (c[col] - bank[slot_client[row]][col])
//                         then momentum / dampening / nesterov as sgd_kernel, p -= lr * d, bf16 shadow
//                         refreshed in the same pass (sgd_prox_kernel with the proximal term replaced)
//   ddl_scaffold_finish : one thread owns a column quad, reads x[col], c[col] once, and walks the slots
//                         from 0 upward with acc = 0:
//                           t     = (x[col] - y[g][col]) * inv_klr[g]
//                           delta = t - c[col]
//                           bank[slot_client[g]][col] = bank[slot_client[g]][col] + delta
//                           acc   = acc + delta * inv_n
//                         a NaN / Inf delta leaves that bank entry untouched and adds nothing;
//                         dc[col] = acc, and with apply_c also c[col] = c[col] + acc (the c loaded
//                         before the loop). The slots' rows must be distinct bank rows (the host
//                         validates the table where it builds it). (3G + 3) P floats moved: y, bank
//                         read, bank write per slot; x, c read, dc written (+ P with apply_c).
//
// Both stream: grid-stride, 256 threads, 16-B accesses where every base pointer is 16-B aligned and
// every row stride a multiple of 4 floats (the scalar path otherwise, the same bits), every add,
// subtract and multiply rounded on its own (no contraction), no LDS, no atomics, no scratch.
#include "ddl_common.h"

struct SGDScaffoldArgs {
  float* p; const float* g; float* mom; bf16_t* shadow; const float* c; const float* bank;
  const int* slot_client;
  long long rows, P, ld;
  float lr, wd, momentum, dampening, grad_scale;
  int nesterov, first_step;
};

__device__ __forceinline__ float scaffold_update(const SGDScaffoldArgs& a, float p, float g, float c, float ci,
                                                 float& m) {
#pragma clang fp contract(off)
  float d = g * a.grad_scale + a.wd * p;
  d = d + (c - ci);
  if (a.momentum != 0.f) {
    m = a.first_step ? d : a.momentum * m + (1.f - a.dampening) * d;
    d = a.nesterov ? d + a.momentum * m : m;
  }
  return p - a.lr * d;
}

__global__ __launch_bounds__(256) void sgd_scaffold_kernel(SGDScaffoldArgs a) {
#pragma clang fp contract(off)
  const long long n = a.rows * a.P;
  const bool has_mom = a.mom && a.momentum != 0.f;
  const bool ld_mom = has_mom && !a.first_step;
  // 16-B path only when no quad straddles a row and every base and bank row is aligned (the
  // shadow's 8-B store too)
  const bool vec = (a.P % 4) == 0 && (a.ld % 4) == 0 &&
                   (((uintptr_t)a.p | (uintptr_t)a.g | (uintptr_t)a.mom | (uintptr_t)a.c | (uintptr_t)a.bank) & 15) == 0 &&
                   ((uintptr_t)a.shadow & 7) == 0;
  for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t * 4 < n;
       t += (long long)gridDim.x * blockDim.x) {
    const long long e = t * 4;
    if (vec) {  // P % 4 == 0: n % 4 == 0, the quad is whole and lies in one row
      const long long row = e / a.P, col = e - row * a.P;
      const float* bank = a.bank + (long long)a.slot_client[row] * a.ld + col;
      float4 pv = *(const float4*)(a.p + e);
      const float4 gv = *(const float4*)(a.g + e);
      const float4 cv = *(const float4*)(a.c + col);
      const float4 bv = *(const float4*)bank;
      float4 mv = ld_mom ? *(const float4*)(a.mom + e) : make_float4(0, 0, 0, 0);
      pv.x = scaffold_update(a, pv.x, gv.x, cv.x, bv.x, mv.x);
      pv.y = scaffold_update(a, pv.y, gv.y, cv.y, bv.y, mv.y);
      pv.z = scaffold_update(a, pv.z, gv.z, cv.z, bv.z, mv.z);
      pv.w = scaffold_update(a, pv.w, gv.w, cv.w, bv.w, mv.w);
      *(float4*)(a.p + e) = pv;
      if (has_mom) *(float4*)(a.mom + e) = mv;
      if (a.shadow) {
        i2v o;
        o[0] = (int)pack_bf2(pv.x, pv.y);
        o[1] = (int)pack_bf2(pv.z, pv.w);
        *(i2v*)(a.shadow + e) = o;
      }
    } else {
      for (long long k = e; k < min(n, e + 4); ++k) {
        const long long row = k / a.P, col = k - row * a.P;
        float m = ld_mom ? a.mom[k] : 0.f;
        const float p = scaffold_update(a, a.p[k], a.g[k], a.c[col],
                                        a.bank[(long long)a.slot_client[row] * a.ld + col], m);
        a.p[k] = p;
        if (has_mom) a.mom[k] = m;
        if (a.shadow) a.shadow[k] = f2bf(p);
      }
    }
  }
}

DDL_API int ddl_sgd_scaffold(const SGDScaffoldArgs* a, hipStream_t s) {
  if (a->rows < 1 || a->P < 1 || a->ld < a->P || !a->p || !a->g || !a->c || !a->bank || !a->slot_client)
    return (int)hipErrorInvalidValue;
  if (a->momentum != 0.f && !a->mom) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(sgd_scaffold_kernel, dim3(grid_for((a->rows * a->P + 3) / 4, 256)), dim3(256), 0, s, *a);
  return (int)hipGetLastError();
}

DDL_API int ddl_sgd_scaffold_args_size() { return (int)sizeof(SGDScaffoldArgs); }

// ------------------------------------------------------------------------------ round-end update
// One coordinate of one slot. Returns false (bank entry and acc untouched) for a NaN / Inf delta.
__device__ __forceinline__ bool finish_update(float x, float y, float k, float c, float inv_n, float& b, float& acc) {
#pragma clang fp contract(off)
  const float t = (x - y) * k;
  const float delta = t - c;
  if ((__float_as_uint(delta) & 0x7f800000u) == 0x7f800000u) return false;
  b = b + delta;
  acc = acc + delta * inv_n;
  return true;
}

// x and dc alias nothing else; the rows y alias no bank row; c is read before it is written by the
// same thread
__global__ __launch_bounds__(256) void scaffold_finish_kernel(const float* __restrict__ y, long long ldy,
                                                              const float* __restrict__ x, float* c, float* bank,
                                                              long long ld, const int* __restrict__ slot_client,
                                                              const float* __restrict__ inv_klr, int G, float inv_n,
                                                              float* dc, long long P, int apply_c) {
#pragma clang fp contract(off)
  const bool vec = (ldy % 4) == 0 && (ld % 4) == 0 &&
                   (((uintptr_t)y | (uintptr_t)x | (uintptr_t)c | (uintptr_t)bank | (uintptr_t)dc) & 15) == 0;
  for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t * 4 < P;
       t += (long long)gridDim.x * blockDim.x) {
    const long long e = t * 4;
    if (e + 4 <= P && vec) {
      const float4 xv = *(const float4*)(x + e), cv = *(const float4*)(c + e);
      float4 acc = make_float4(0, 0, 0, 0);
      // four slots at a time: their loads are issued before the first bank store (the slots' bank
      // rows are distinct), the updates then run in slot order
      for (int g0 = 0; g0 < G; g0 += 4) {
        float4 yv[4], bv[4];
        float k[4];
        float* bp[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (g0 + j < G) {
            bp[j] = bank + (long long)slot_client[g0 + j] * ld + e;
            yv[j] = *(const float4*)(y + (g0 + j) * ldy + e);
            bv[j] = *(const float4*)bp[j];
            k[j] = inv_klr[g0 + j];
          }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (g0 + j < G) {
            // a skipped coordinate stores back the bits it loaded
            finish_update(xv.x, yv[j].x, k[j], cv.x, inv_n, bv[j].x, acc.x);
            finish_update(xv.y, yv[j].y, k[j], cv.y, inv_n, bv[j].y, acc.y);
            finish_update(xv.z, yv[j].z, k[j], cv.z, inv_n, bv[j].z, acc.z);
            finish_update(xv.w, yv[j].w, k[j], cv.w, inv_n, bv[j].w, acc.w);
            *(float4*)bp[j] = bv[j];
          }
        }
      }
      *(float4*)(dc + e) = acc;
      if (apply_c) {
        float4 o;
        o.x = cv.x + acc.x; o.y = cv.y + acc.y; o.z = cv.z + acc.z; o.w = cv.w + acc.w;
        *(float4*)(c + e) = o;
      }
    } else {
      for (long long i = e; i < min(P, e + 4); ++i) {
        const float xi = x[i], ci = c[i];
        float acc = 0.f;
        for (int g = 0; g < G; ++g) {
          float* bp = bank + (long long)slot_client[g] * ld + i;
          float b = *bp;
          if (finish_update(xi, y[g * ldy + i], inv_klr[g], ci, inv_n, b, acc)) *bp = b;
        }
        dc[i] = acc;
        if (apply_c) c[i] = ci + acc;
      }
    }
  }
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
