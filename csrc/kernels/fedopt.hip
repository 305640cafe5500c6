// Remedies for client drift under non-IID data [north-star, absent in reference]: the corrected
// local step of FedProx (Li et al. 2020) and SCAFFOLD (Karimireddy et al. 2020), and the FedOpt
// server optimizers (Reddi et al. 2021, Algorithm 2; FedAvgM of Hsu et al. 2019).
//
//   ddl_sgd_corrected   : rows p/g/mom/shadow [G][P]: d = g * grad_scale + wd * p, d = d + term, then
//                         momentum / dampening / nesterov as sgd_kernel, p -= lr * d, bf16 shadow
//                         refreshed in the same pass. One kernel template, an instance per term:
//                           SGD_PROX    : mu * (p - ref[col]), ref the anchor [P] (the round's w_global)
//                           SGD_CONTROL : ref[col] - bank[slot_client[row]][col], ref the server's control
//                                         variate c [P], client i's in row i of bank [N][ld], read in
//                                         place through the int32 device table slot_client [G] (so a
//                                         captured round graph keeps its pointers and the next round
//                                         only overwrites the table's contents)
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
// All three stream on quad_stream (quad_stream.h): grid-stride, 256 threads, 16-B accesses where
// every base pointer and row stride is 16-B aligned, element by element otherwise, one body for
// both; every add, multiply, divide and sqrtf rounded on its own (no contraction), no LDS, no
// atomics, no scratch.
#include "quad_stream.h"

enum { SGD_PROX = 0, SGD_CONTROL = 1 };

struct SGDCorrectedArgs {
  float* p; const float* g; float* mom; bf16_t* shadow;
  const float* ref;                             // [P]: the anchor (SGD_PROX), the server's c (SGD_CONTROL)
  const float* bank; const int* slot_client;    // SGD_CONTROL: clients' rows [N][ld], slot -> client
  long long rows, P, ld;
  float lr, wd, momentum, dampening, grad_scale, mu;
  int nesterov, first_step, correction;
};

// The correction terms: what the step adds to d for the elements [col, col + W) of slot `row`, and
// what has to be aligned beyond p, g, mom and P for the 16-B path.
struct ProxTerm {  // mu * (p - anchor[col])
  static __device__ __forceinline__ bool aligned(const SGDCorrectedArgs& a) { return ((uintptr_t)a.ref & 15) == 0; }
  template <int W>
  static __device__ __forceinline__ fvec<W> term(const SGDCorrectedArgs& a, long long, long long col, const fvec<W>& p) {
#pragma clang fp contract(off)
    const fvec<W> anc = ldv<W>(a.ref + col);
    fvec<W> t;
#pragma unroll
    for (int i = 0; i < W; ++i) t[i] = a.mu * (p[i] - anc[i]);
    return t;
  }
};

struct ControlTerm {  // c[col] - bank[slot_client[row]][col]
  static __device__ __forceinline__ bool aligned(const SGDCorrectedArgs& a) {
    return (a.ld % 4) == 0 && (((uintptr_t)a.ref | (uintptr_t)a.bank) & 15) == 0;
  }
  template <int W>
  static __device__ __forceinline__ fvec<W> term(const SGDCorrectedArgs& a, long long row, long long col, const fvec<W>&) {
#pragma clang fp contract(off)
    const fvec<W> c = ldv<W>(a.ref + col);
    const fvec<W> ci = ldv<W>(a.bank + (long long)a.slot_client[row] * a.ld + col);
    fvec<W> t;
#pragma unroll
    for (int i = 0; i < W; ++i) t[i] = c[i] - ci[i];
    return t;
  }
};

template <class Term>
__global__ __launch_bounds__(256) void sgd_corrected_kernel(SGDCorrectedArgs a) {
  const long long n = a.rows * a.P;
  const bool has_mom = a.mom && a.momentum != 0.f;
  const bool ld_mom = has_mom && !a.first_step;
  // 16-B path only when no quad straddles a row (P % 4 == 0: n % 4 == 0, every quad is whole and
  // lies in one row) and every base is aligned (the shadow's 8-B store too)
  const bool vec = (a.P % 4) == 0 && (((uintptr_t)a.p | (uintptr_t)a.g | (uintptr_t)a.mom) & 15) == 0 &&
                   ((uintptr_t)a.shadow & 7) == 0 && Term::aligned(a);
  quad_stream(n, vec, [&](long long e, auto w) {
#pragma clang fp contract(off)
    constexpr int W = decltype(w)::value;
    const long long row = e / a.P, col = e - row * a.P;
    fvec<W> p = ldv<W>(a.p + e);
    const fvec<W> g = ldv<W>(a.g + e);
    const fvec<W> t = Term::template term<W>(a, row, col, p);
    fvec<W> m = ld_mom ? ldv<W>(a.mom + e) : fzero<W>();
#pragma unroll
    for (int i = 0; i < W; ++i) {
      float d = g[i] * a.grad_scale + a.wd * p[i];
      d = d + t[i];
      if (a.momentum != 0.f) {
        m[i] = a.first_step ? d : a.momentum * m[i] + (1.f - a.dampening) * d;
        d = a.nesterov ? d + a.momentum * m[i] : m[i];
      }
      p[i] = p[i] - a.lr * d;
    }
    stv<W>(a.p + e, p);
    if (has_mom) stv<W>(a.mom + e, m);
    if (a.shadow) stv_bf16<W>(a.shadow + e, p);
  });
}

DDL_API int ddl_sgd_corrected(const SGDCorrectedArgs* a, hipStream_t s) {
  if (a->rows < 1 || a->P < 1 || !a->p || !a->g || !a->ref) return (int)hipErrorInvalidValue;
  if (a->momentum != 0.f && !a->mom) return (int)hipErrorInvalidValue;
  const dim3 grid(grid_for((a->rows * a->P + 3) / 4, 256));
  if (a->correction == SGD_PROX) {
    hipLaunchKernelGGL(sgd_corrected_kernel<ProxTerm>, grid, dim3(256), 0, s, *a);
  } else if (a->correction == SGD_CONTROL) {
    if (!a->bank || !a->slot_client || a->ld < a->P) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(sgd_corrected_kernel<ControlTerm>, grid, dim3(256), 0, s, *a);
  } else {
    return (int)hipErrorInvalidValue;
  }
  return (int)hipGetLastError();
}

DDL_API int ddl_sgd_corrected_args_size() { return (int)sizeof(SGDCorrectedArgs); }

// ------------------------------------------------------------------------------ server optimizers
enum { SOPT_SGDM = 0, SOPT_ADAGRAD = 1, SOPT_ADAM = 2, SOPT_YOGI = 3 };

struct ServerOptHyper {
  float lr, beta1, beta2, tau;
  int kind, x_is_delta;
};

// One coordinate, every operation rounded on its own in the order of the header comment; a NaN /
// Inf delta leaves w, m, v untouched.
__device__ __forceinline__ void server_update(const ServerOptHyper& h, float x, float& w, float& m, float& v) {
#pragma clang fp contract(off)
  const float d = h.x_is_delta ? x : x - w;
  if ((__float_as_uint(d) & 0x7f800000u) == 0x7f800000u) return;
  if (h.kind == SOPT_SGDM) {
    m = h.beta1 * m + d;
    w = w + h.lr * m;
    return;
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
}

// The step on W coordinates whose state the caller loaded (before its row loop, so the loads are in
// flight with it); a skipped coordinate stores back the bits it loaded.
template <int W>
__device__ __forceinline__ void server_step(const ServerOptHyper& h, const fvec<W>& x, fvec<W> wv, fvec<W> mv,
                                            fvec<W> vv, float* w, float* m, float* v, long long e) {
#pragma unroll
  for (int i = 0; i < W; ++i) server_update(h, x[i], wv[i], mv[i], vv[i]);
  stv<W>(w + e, wv);
  stv<W>(m + e, mv);
  if (h.kind != SOPT_SGDM) stv<W>(v + e, vv);
}

// x may alias nothing it writes: w, m, v are read before they are written by the same thread
__global__ __launch_bounds__(256) void server_opt_kernel(float* w, const float* __restrict__ x, float* m, float* v,
                                                         long long n, ServerOptHyper h) {
  const bool vec = (((uintptr_t)w | (uintptr_t)x | (uintptr_t)m | (uintptr_t)v) & 15) == 0;
  quad_stream(n, vec, [&](long long e, auto wd) {
    constexpr int W = decltype(wd)::value;
    const fvec<W> wv = ldv<W>(w + e), mv = ldv<W>(m + e);
    const fvec<W> vv = v ? ldv<W>(v + e) : fzero<W>();
    server_step<W>(h, ldv<W>(x + e), wv, mv, vv, w, m, v, e);
  });
}

__global__ __launch_bounds__(256) void server_opt_rows_kernel(const float* __restrict__ rows, long long ld,
                                                              const float* __restrict__ coeff, int G, float* w,
                                                              float* m, float* v, long long n, ServerOptHyper h) {
  const bool vec = (ld % 4) == 0 &&
                   (((uintptr_t)rows | (uintptr_t)w | (uintptr_t)m | (uintptr_t)v) & 15) == 0;
  quad_stream(n, vec, [&](long long e, auto wd) {
    constexpr int W = decltype(wd)::value;
    const fvec<W> wv = ldv<W>(w + e), mv = ldv<W>(m + e);
    const fvec<W> vv = v ? ldv<W>(v + e) : fzero<W>();
    fvec<W> acc = fzero<W>();  // weighted_sum_kernel's sum, from 0
    add_weighted_rows<W>(acc, rows, ld, coeff, G, e);
    server_step<W>(h, acc, wv, mv, vv, w, m, v, e);
  });
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
