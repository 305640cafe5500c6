// Remedies for client drift under non-IID data [north-star, absent in reference]: the FedProx local
// step (Li et al. 2020) and the FedOpt server optimizers (Reddi et al. 2021, Algorithm 2; FedAvgM
// of Hsu et al. 2019).
//
//   ddl_sgd_prox        : rows p/g/mom/shadow [G][P], one anchor a [P] (the round's w_global):
//                         d = g * grad_scale + wd * p + mu * (p - a[col]), then momentum / dampening /
//                         nesterov as sgd_kernel, p -= lr * d, bf16 shadow refreshed in the same pass
//   ddl_server_opt      : delta = x_is_delta ? x : x - w, then in place on w, m, v [n]
//                           sgdm    : m = b1 * m + delta                   w = w + lr * m
//                           adagrad : m = b1 * m + (1 - b1) * delta        v = v + delta * delta
//                           adam    :   "                                  v = b2 * v + (1 - b2) * delta * delta
//                           yogi    :   "              v = v - (1 - b2) * (delta * delta) * sign(v - delta * delta)
//                                                                          w = w + lr * m / (sqrtf(v) + tau)
//                         no bias correction; a coordinate whose delta is NaN / Inf keeps its w, m, v
//   ddl_server_opt_rows : x = sum_g coeff[g] * rows[g] formed in registers in weighted_sum_kernel's
//                         order (products rounded, added in client order from 0), then the same
//                         update: the bits of ddl_weighted_sum into a temporary + ddl_server_opt,
//                         moving (G + 6) n floats in one launch instead of (G + 8) n in two
//                         (G + 4 against G + 6 for sgdm, which has no v)
//
// All three stream: grid-stride, 256 threads, 16-B accesses where every base pointer and row stride
// is 16-B aligned (the scalar path otherwise, the same bits), every add, multiply, divide and sqrtf
// rounded on its own (no contraction), no LDS, no atomics, no scratch.
#include "ddl_common.h"

struct SGDProxArgs {
  float* p; const float* g; float* mom; bf16_t* shadow; const float* anchor;
  long long rows, P;
  float lr, wd, momentum, dampening, grad_scale, mu;
  int nesterov, first_step;
};

__device__ __forceinline__ float prox_update(const SGDProxArgs& a, float p, float g, float anc, float& m) {
#pragma clang fp contract(off)
  float d = g * a.grad_scale + a.wd * p;
  d = d + a.mu * (p - anc);
  if (a.momentum != 0.f) {
    m = a.first_step ? d : a.momentum * m + (1.f - a.dampening) * d;
    d = a.nesterov ? d + a.momentum * m : m;
  }
  return p - a.lr * d;
}

__global__ __launch_bounds__(256) void sgd_prox_kernel(SGDProxArgs a) {
#pragma clang fp contract(off)
  const long long n = a.rows * a.P;
  const bool has_mom = a.mom && a.momentum != 0.f;
  const bool ld_mom = has_mom && !a.first_step;
  // 16-B path only when no quad straddles a row and every base is aligned (the shadow's 8-B store too)
  const bool vec = (a.P % 4) == 0 &&
                   (((uintptr_t)a.p | (uintptr_t)a.g | (uintptr_t)a.mom | (uintptr_t)a.anchor) & 15) == 0 &&
                   ((uintptr_t)a.shadow & 7) == 0;
  for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t * 4 < n;
       t += (long long)gridDim.x * blockDim.x) {
    const long long e = t * 4;
    if (vec) {  // P % 4 == 0: n % 4 == 0, the quad is whole and lies in one row
      const long long col = e % a.P;
      float4 pv = *(const float4*)(a.p + e);
      const float4 gv = *(const float4*)(a.g + e);
      const float4 av = *(const float4*)(a.anchor + col);
      float4 mv = ld_mom ? *(const float4*)(a.mom + e) : make_float4(0, 0, 0, 0);
      pv.x = prox_update(a, pv.x, gv.x, av.x, mv.x);
      pv.y = prox_update(a, pv.y, gv.y, av.y, mv.y);
      pv.z = prox_update(a, pv.z, gv.z, av.z, mv.z);
      pv.w = prox_update(a, pv.w, gv.w, av.w, mv.w);
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
        float m = ld_mom ? a.mom[k] : 0.f;
        const float p = prox_update(a, a.p[k], a.g[k], a.anchor[k % a.P], m);
        a.p[k] = p;
        if (has_mom) a.mom[k] = m;
        if (a.shadow) a.shadow[k] = f2bf(p);
      }
    }
  }
}

DDL_API int ddl_sgd_prox(const SGDProxArgs* a, hipStream_t s) {
  if (a->rows < 1 || a->P < 1 || !a->p || !a->g || !a->anchor) return (int)hipErrorInvalidValue;
  if (a->momentum != 0.f && !a->mom) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(sgd_prox_kernel, dim3(grid_for((a->rows * a->P + 3) / 4, 256)), dim3(256), 0, s, *a);
  return (int)hipGetLastError();
}

DDL_API int ddl_sgd_prox_args_size() { return (int)sizeof(SGDProxArgs); }

// ------------------------------------------------------------------------------ server optimizers
enum { SOPT_SGDM = 0, SOPT_ADAGRAD = 1, SOPT_ADAM = 2, SOPT_YOGI = 3 };

struct ServerOptHyper {
  float lr, beta1, beta2, tau;
  int kind, x_is_delta;
};

// One coordinate, every operation rounded on its own in the order of the header comment. Returns
// false (w, m, v untouched) for a NaN / Inf delta.
__device__ __forceinline__ bool server_update(const ServerOptHyper& h, float x, float& w, float& m, float& v) {
#pragma clang fp contract(off)
  const float d = h.x_is_delta ? x : x - w;
  if ((__float_as_uint(d) & 0x7f800000u) == 0x7f800000u) return false;
  if (h.kind == SOPT_SGDM) {
    m = h.beta1 * m + d;
    w = w + h.lr * m;
    return true;
  }
  const float omb1 = 1.f - h.beta1, omb2 = 1.f - h.beta2;
  m = h.beta1 * m + omb1 * d;
  if (h.kind == SOPT_ADAGRAD) {
    v = v + d * d;
  } else if (h.kind == SOPT_ADAM) {
    v = h.beta2 * v + omb2 * d * d;
  } else {
    const float d2 = d * d;
    const float diff = v - d2;
    const float sgn = diff > 0.f ? 1.f : (diff < 0.f ? -1.f : 0.f);
    v = v - omb2 * d2 * sgn;
  }
  w = w + h.lr * m / (sqrtf(v) + h.tau);
  return true;
}

// the quad's state, loaded by the caller (before its row loop, so the loads are in flight with it)
__device__ __forceinline__ void server_update4(const ServerOptHyper& h, const float4& x, float4 wv, float4 mv,
                                               float4 vv, float* w, float* m, float* v, long long e) {
  const bool has_v = h.kind != SOPT_SGDM;
  // a skipped coordinate stores back the bits it loaded
  server_update(h, x.x, wv.x, mv.x, vv.x);
  server_update(h, x.y, wv.y, mv.y, vv.y);
  server_update(h, x.z, wv.z, mv.z, vv.z);
  server_update(h, x.w, wv.w, mv.w, vv.w);
  *(float4*)(w + e) = wv;
  *(float4*)(m + e) = mv;
  if (has_v) *(float4*)(v + e) = vv;
}

__device__ __forceinline__ void server_update1(const ServerOptHyper& h, float x, float* w, float* m, float* v,
                                               long long k) {
  const bool has_v = h.kind != SOPT_SGDM;
  float wk = w[k], mk = m[k], vk = has_v ? v[k] : 0.f;
  if (server_update(h, x, wk, mk, vk)) {
    w[k] = wk;
    m[k] = mk;
    if (has_v) v[k] = vk;
  }
}

// x may alias nothing it writes: w, m, v are read before they are written by the same thread
__global__ __launch_bounds__(256) void server_opt_kernel(float* w, const float* __restrict__ x, float* m, float* v,
                                                         long long n, ServerOptHyper h) {
#pragma clang fp contract(off)
  const bool vec = (((uintptr_t)w | (uintptr_t)x | (uintptr_t)m | (uintptr_t)v) & 15) == 0;
  for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t * 4 < n;
       t += (long long)gridDim.x * blockDim.x) {
    const long long e = t * 4;
    if (e + 4 <= n && vec) {
      const float4 wv = *(const float4*)(w + e), mv = *(const float4*)(m + e);
      const float4 vv = v ? *(const float4*)(v + e) : make_float4(0, 0, 0, 0);
      server_update4(h, *(const float4*)(x + e), wv, mv, vv, w, m, v, e);
    } else {
      for (long long k = e; k < min(n, e + 4); ++k) server_update1(h, x[k], w, m, v, k);
    }
  }
}

__global__ __launch_bounds__(256) void server_opt_rows_kernel(const float* __restrict__ rows, long long ld,
                                                              const float* __restrict__ coeff, int G, float* w,
                                                              float* m, float* v, long long n, ServerOptHyper h) {
#pragma clang fp contract(off)
  const bool vec = (ld % 4) == 0 &&
                   (((uintptr_t)rows | (uintptr_t)w | (uintptr_t)m | (uintptr_t)v) & 15) == 0;
  for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t * 4 < n;
       t += (long long)gridDim.x * blockDim.x) {
    const long long e = t * 4;
    if (e + 4 <= n && vec) {
      const float4 wv = *(const float4*)(w + e), mv = *(const float4*)(m + e);
      const float4 vv = v ? *(const float4*)(v + e) : make_float4(0, 0, 0, 0);
      // weighted_sum_kernel's sum: from 0, products rounded, added in client order
      float4 acc = make_float4(0, 0, 0, 0);
      for (int g = 0; g < G; ++g) {
        const float c = coeff[g];
        const float4 r = *(const float4*)(rows + g * ld + e);
        acc.x = acc.x + c * r.x; acc.y = acc.y + c * r.y;
        acc.z = acc.z + c * r.z; acc.w = acc.w + c * r.w;
      }
      server_update4(h, acc, wv, mv, vv, w, m, v, e);
    } else {
      for (long long k = e; k < min(n, e + 4); ++k) {
        float acc = 0.f;
        for (int g = 0; g < G; ++g) acc = acc + coeff[g] * rows[g * ld + k];
        server_update1(h, acc, w, m, v, k);
      }
    }
  }
}

static bool server_opt_args_ok(const float* w, const float* m, const float* v, long long n, int kind, float lr,
                               float tau) {
  if (!w || !m || n < 1 || kind < SOPT_SGDM || kind > SOPT_YOGI) return false;
  if (kind != SOPT_SGDM && (!v || !(tau > 0.f))) return false;
  return lr > 0.f;
}

DDL_API int ddl_server_opt(float* w, const float* x, float* m, float* v, long long n, int kind, int x_is_delta,
                           float lr, float beta1, float beta2, float tau, hipStream_t s) {
  if (!x || !server_opt_args_ok(w, m, v, n, kind, lr, tau)) return (int)hipErrorInvalidValue;
  const ServerOptHyper h = {lr, beta1, beta2, tau, kind, x_is_delta != 0};
  hipLaunchKernelGGL(server_opt_kernel, dim3(grid_for((n + 3) / 4, 256)), dim3(256), 0, s, w, x, m,
                     kind == SOPT_SGDM ? nullptr : v, n, h);
  return (int)hipGetLastError();
}

DDL_API int ddl_server_opt_rows(const float* rows, long long ld, const float* coeff, int G, float* w, float* m,
                                float* v, long long n, int kind, int x_is_delta, float lr, float beta1,
                                float beta2, float tau, hipStream_t s) {
  if (!rows || !coeff || G < 1 || (G > 1 && ld < n) || !server_opt_args_ok(w, m, v, n, kind, lr, tau))
    return (int)hipErrorInvalidValue;
  const ServerOptHyper h = {lr, beta1, beta2, tau, kind, x_is_delta != 0};
  hipLaunchKernelGGL(server_opt_rows_kernel, dim3(grid_for((n + 3) / 4, 256)), dim3(256), 0, s, rows, ld,
                     coeff, G, w, m, kind == SOPT_SGDM ? nullptr : v, n, h);
  return (int)hipGetLastError();
}
