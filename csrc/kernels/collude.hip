// Colluding model-poisoning attacks [north-star, absent in reference]: every attacker sends the same
// vector, built from per-coordinate statistics of other clients' updates u_k = fl32(x_k - c).
//
//   mode 0, ALIE ("A Little Is Enough", Baruch et al. 2019): p_i = fl32(mu_i - coef * sigma_i)
//   mode 1, IPM  (inner-product manipulation, Xie et al. 2019): p_i = fl32(-coef * mu_i)
//
// mu_i and sigma_i (the population std) are taken over the ns source rows named by src_rows, in table
// order, over the finite d = fl32(src[src_rows[j]][i] - c_i) alone; a coordinate without a finite
// source gives p_i = 0. Every destination row gets c_i + p_i (one fp32 add; p_i without a centre).
//
// The moments are one pass in double on values shifted by the coordinate's first finite d:
// t = d - shift, s1 += t, s2 += t * t, mu = shift + s1 / m, var = max(0, (s2 - s1 * s1 / m) / m).
// Unshifted, s2 - s1^2 / m cancels to a relative error of about (mu / sigma)^2 * 2^-53, and identical
// rows would leave a sigma of rounding noise; shifted, t is exactly 0 for them (sigma == 0 exactly)
// and |t| is of the order of sigma otherwise. Nothing is held per row, so ns is unbounded.
//
// One stream on quad_stream: one read of the ns rows and the centre, one write of the nd rows, no
// atomics, no LDS.
#include "quad_stream.h"

// src and dst may be the same buffer and dst_rows may name source rows: a thread reads all the
// sources of its coordinates before it writes them, and no other thread touches those coordinates
// (hence no __restrict__ on either).
__global__ void collude_kernel(const float* src, long long ld_s, const int* __restrict__ src_rows, int ns,
                               const float* __restrict__ center, float* dst, long long ld_d,
                               const int* __restrict__ dst_rows, int nd, long long n, int mode, double coef) {
  const bool vec = (ld_s % 4) == 0 && (ld_d % 4) == 0 &&
                   (((uintptr_t)src | (uintptr_t)dst | (uintptr_t)center) & 15) == 0;
  quad_stream(n, vec, [&](long long e, auto w) {
#pragma clang fp contract(off)
    constexpr int W = decltype(w)::value;
    const fvec<W> c = center ? ldv<W>(center + e) : fzero<W>();
    double shift[W], s1[W], s2[W];
    int m[W];
#pragma unroll
    for (int i = 0; i < W; ++i) { shift[i] = 0.0; s1[i] = 0.0; s2[i] = 0.0; m[i] = 0; }
    for (int j = 0; j < ns; ++j) {
      const fvec<W> v = ldv<W>(src + src_rows[j] * ld_s + e);
#pragma unroll
      for (int i = 0; i < W; ++i) {
        const float d = v[i] - c[i];
        if (fabsf(d) < INFINITY) {  // false for NaN and +-inf: the entry is skipped
          if (m[i] == 0) shift[i] = (double)d;
          const double t = (double)d - shift[i];
          s1[i] = s1[i] + t;
          s2[i] = s2[i] + t * t;
          m[i] += 1;
        }
      }
    }
    fvec<W> o;
#pragma unroll
    for (int i = 0; i < W; ++i) {
      float p = 0.f;
      if (m[i] > 0) {
        const double cnt = (double)m[i];
        const double mu = shift[i] + s1[i] / cnt;
        if (mode == 0) {
          const double var = fmax(0.0, (s2[i] - s1[i] * s1[i] / cnt) / cnt);
          p = (float)(mu - coef * sqrt(var));
        } else {
          p = (float)(-coef * mu);
        }
      }
      o[i] = center ? c[i] + p : p;
    }
    for (int t = 0; t < nd; ++t) stv<W>(dst + dst_rows[t] * ld_d + e, o);
  });
}

DDL_API int ddl_collude(const float* src, long long ld_s, const int* src_rows, int ns, const float* center,
                        float* dst, long long ld_d, const int* dst_rows, int nd, long long n, int mode,
                        double coef, hipStream_t s) {
  if (ns < 0 || nd < 1 || n < 1 || mode < 0 || mode > 1) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(collude_kernel, dim3(grid_for((n + 3) / 4, 256)), dim3(256), 0, s, src, ld_s, src_rows,
                     ns, center, dst, ld_d, dst_rows, nd, n, mode, coef);
  return (int)hipGetLastError();
}
