// Clipped FedAvg aggregation: the norm-bounding defence (Sun et al. 2019) and DP-FedAvg
// (McMahan et al. 2018) [north-star, absent in reference]. Each client update u_k = x_k - c is
// scaled to L2 norm at most C before the weighted mean; DP-FedAvg adds N(0, std^2) to the result.
//
//   ddl_update_sqnorm : sq[k] = sum_i fl32(x_ki - c_i)^2, squares accumulated in double
//   ddl_clip_scales   : norms[k] = sqrt(sq[k]), cs[k] = coeff[k] * min(1, C / norms[k]);
//                       cs[k] = 0 for a row whose squared norm is NaN / Inf
//   ddl_clipped_sum   : delta[i] (+)= sum_k cs[k] * fl32(x_ki - c_i), rows with cs[k] == 0 not read
//   ddl_rlr_sum       : the clipped sum and the per-coordinate sign vote of the robust learning rate
//                       in one read of the rows; delta[i] negated where |votes[i]| < theta
//   ddl_rlr_flip      : that negation on its own, after the cross-rank sums of delta and votes
//   ddl_apply_update  : w[i] = c[i] + delta[i] + std * z_i, z_i ~ N(0, 1) from Philox
//   ddl_cc_step       : one centered-clipping iteration, v += sum_k cs[k] * fl32(x_k - ctr), fused
//                       with the next iteration's squared norms (up to 16 rows, see there)
//   ddl_gm_scales     : the row scales of one smoothed Weiszfeld iteration (geometric median / RFA),
//                       cs[k] = (coeff[k] / max(nu, norms[k])) / their sum; the step itself is ddl_cc_step
//   ddl_root_dots     : FLTrust: dots[k] = <d_k, d_0> and sq[k] = |d_k|^2 against the server's root
//                       update d_0 in one read of the rows, in double (see there)
//   ddl_trust_scales  : cs[k] = coeff[k] * relu(cos(d_k, d_0)) * (|d_0| / |d_k|) / the sum of the trusts
//
// All four stream: two reads of the client rows (norms, then the sum), no LDS tiling, no scratch,
// no float atomics, and no block waits for another: the per-block partial squared norms go out with
// plain stores and a tiny second launch folds them in a fixed order, so the norms (and with them
// the whole aggregate) are bit-reproducible. G is bounded by memory only. The squared norms and the
// sum run on quad_stream (quad_stream.h): 16-B loads where every row start is 16-B aligned, element
// by element otherwise, one body for both; apply_update keeps a loop of its own (see there).
#include "quad_stream.h"

// blocks along a row for the squared norms: about 2048 blocks in all over the G rows (256 CUs x 8
// resident blocks, the rest by the grid-stride loop). Measured at 8 rows x 11.2M with a centre:
// 0.068 ms at 256 blocks per row, 0.095 at 1024, 0.101 at 2048 and 8192 -- every block ends in a
// reduction and a barrier, so few long blocks beat many short ones.
static int sqnorm_row_blocks(int G, long long n) {
  const int bx = grid_for((n + 3) / 4, 256);
  const int lim = G >= 2048 ? 1 : 2048 / (G < 1 ? 1 : G);
  return bx < lim ? bx : lim;
}

__global__ __launch_bounds__(256) void update_sqnorm_kernel(const float* __restrict__ X, long long ld,
                                                            const float* __restrict__ c, int G, long long n,
                                                            double* __restrict__ part) {
#pragma clang fp contract(off)
  __shared__ double red[4];
  // quads only when every row start and the centre are 16-B aligned
  const bool vec = (ld % 4) == 0 && (((uintptr_t)X | (uintptr_t)c) & 15) == 0;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  for (int g = blockIdx.y; g < G; g += gridDim.y) {
    const float* row = X + (long long)g * ld;
    // the difference rounded to fp32 (the update as `rows - w_global` forms it), its square exact
    // in double and added in double from the first add
    double acc = 0.0;
    quad_stream(n, vec, [&](long long e, auto w) {
#pragma clang fp contract(off)
      constexpr int W = decltype(w)::value;
      const fvec<W> v = ldv<W>(row + e);
      const fvec<W> m = c ? ldv<W>(c + e) : fzero<W>();
#pragma unroll
      for (int i = 0; i < W; ++i) {
        const float d = v[i] - m[i];
        acc += (double)d * (double)d;
      }
    });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (lane == 0) red[wid] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[(long long)g * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
    __syncthreads();  // red is reused by the block's next row
  }
}

// sq[g] = the row's bx partials: thread t adds partials t, t + 256, ... in order, then a fixed LDS
// tree (the order depends on bx alone)
__global__ __launch_bounds__(256) void sqnorm_fold_kernel(const double* __restrict__ part, int bx, int G,
                                                          double* __restrict__ sq) {
  __shared__ double red[256];
  for (int g = blockIdx.x; g < G; g += gridDim.x) {
    const double* p = part + (long long)g * bx;
    double s = 0.0;
    for (int b = threadIdx.x; b < bx; b += 256) s += p[b];
    red[threadIdx.x] = s;
    __syncthreads();
#pragma unroll
    for (int w = 128; w > 0; w >>= 1) {
      if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
      __syncthreads();
    }
    if (threadIdx.x == 0) sq[g] = red[0];
    __syncthreads();
  }
}

// doubles of scratch `ddl_update_sqnorm` needs for G rows of n coordinates
DDL_API long long ddl_update_sqnorm_workspace(int G, long long n) {
  if (G < 1 || n < 1) return 0;
  return (long long)G * sqnorm_row_blocks(G, n);
}

DDL_API int ddl_update_sqnorm(const float* X, long long ld, const float* center, int G, long long n,
                              double* part, long long part_cap, double* sq, hipStream_t s) {
  if (G < 1 || n < 1 || part_cap < ddl_update_sqnorm_workspace(G, n)) return (int)hipErrorInvalidValue;
  const int bx = sqnorm_row_blocks(G, n);
  const int gy = G < 65535 ? G : 65535;
  // one block per row: its partial is the row's squared norm
  hipLaunchKernelGGL(update_sqnorm_kernel, dim3(bx, gy), dim3(256), 0, s, X, ld, center, G, n,
                     bx == 1 ? sq : part);
  if (bx > 1)
    hipLaunchKernelGGL(sqnorm_fold_kernel, dim3(gy), dim3(256), 0, s, part, bx, G, sq);
  return (int)hipGetLastError();
}

// norm_k = sqrt(sq_k) and s_k = min(1, C / norm_k) in double, s_k rounded to fp32 (exactly 1 for
// norm_k <= C, norm_k = 0 included), cs_k = fl32(coeff_k * s_k). A squared norm that is NaN / Inf
// (a NaN / Inf entry in the row) gives cs_k = 0, which the sum kernel takes as "skip the row".
__global__ void clip_scales_kernel(const double* __restrict__ sq, const float* __restrict__ coeff, int G,
                                   double clip, float* __restrict__ norms, float* __restrict__ cs) {
#pragma clang fp contract(off)
  GSTRIDE_LOOP(k, G) {
    const double q = sq[k];
    const double nrm = sqrt(q);
    norms[k] = (float)nrm;  // +inf for a finite row too long for fp32
    float r = 0.f;
    if (q < (double)INFINITY) {  // false for NaN and +inf
      const float sc = (nrm <= clip) ? 1.f : (float)(clip / nrm);
      r = coeff[k] * sc;
    }
    cs[k] = r;
  }
}

DDL_API int ddl_clip_scales(const double* sq, const float* coeff, int G, double clip, float* norms,
                            float* cs, hipStream_t s) {
  if (G < 1 || !(clip > 0.0)) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(clip_scales_kernel, dim3(grid_for(G, 256)), dim3(256), 0, s, sq, coeff, G, clip,
                     norms, cs);
  return (int)hipGetLastError();
}

// The row scales of one smoothed Weiszfeld iteration (geometric median / RFA, Pillutla et al. 2022),
// one block, double throughout: norms[k] = sqrt(sq_k); beta_k = coeff_k / max(nu, sqrt(sq_k)), or
// coeff_k itself with `init` (the weighted mean as the starting point), and 0 for a row whose
// squared norm is NaN / Inf; S = beta_0 + beta_1 + ... added by one thread in index order (the
// betas of 256 rows at a time computed by the block into LDS), so that the ranks' partial S added
// in rank order give the bits of one process holding the rows in that order; beta_sum[0] = S;
// cs[k] = beta_k / T rounded to fp32, T = *total when given (the S of all ranks), else S; T == 0
// (no row left, or all weights 0) gives cs = 0 throughout.
__device__ __forceinline__ double gm_beta(double q, float coeff, double nu, int init) {
  if (!(q < (double)INFINITY)) return 0.0;  // NaN and +inf
  if (init) return (double)coeff;
  const double nrm = sqrt(q);
  return (double)coeff / (nrm > nu ? nrm : nu);
}

__global__ __launch_bounds__(256) void gm_scales_kernel(const double* __restrict__ sq, const float* __restrict__ coeff,
                                                        int G, double nu, int init, const double* __restrict__ total,
                                                        float* __restrict__ norms, float* __restrict__ cs,
                                                        double* __restrict__ beta_sum) {
#pragma clang fp contract(off)
  __shared__ double chunk[256];
  __shared__ double sum;
  const int tid = threadIdx.x;
  double S = 0.0;
  for (int base = 0; base < G; base += 256) {
    const int k = base + tid;
    if (k < G) {
      const double q = sq[k];
      norms[k] = (float)sqrt(q);  // +inf for a finite row too long for fp32
      chunk[tid] = gm_beta(q, coeff[k], nu, init);
    }
    __syncthreads();
    if (tid == 0) {
      const int m = G - base < 256 ? G - base : 256;
      for (int j = 0; j < m; ++j) S += chunk[j];
    }
    __syncthreads();
  }
  if (tid == 0) {
    beta_sum[0] = S;
    sum = total ? *total : S;
  }
  __syncthreads();
  const double T = sum;
  for (int k = tid; k < G; k += 256) cs[k] = (T == 0.0) ? 0.f : (float)(gm_beta(sq[k], coeff[k], nu, init) / T);
}

DDL_API int ddl_gm_scales(const double* sq, const float* coeff, int G, double nu, int init, const double* total,
                          float* norms, float* cs, double* beta_sum, hipStream_t s) {
  if (G < 1 || (!init && !(nu > 0.0))) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(gm_scales_kernel, dim3(1), dim3(256), 0, s, sq, coeff, G, nu, init, total, norms, cs,
                     beta_sum);
  return (int)hipGetLastError();
}

// FLTrust (Cao et al. 2021): every client row against the server's root row in ONE read of the rows.
// With d_k = fl32(x_k - c) and d_0 = fl32(r - c) (the rows themselves without a centre):
//   dots[k] = sum_i d_ki * d_0i,  sq[k] = sum_i d_ki^2  (k < G),  dots[G] = sq[G] = sum_i d_0i^2
// update_sqnorm_kernel's discipline: the difference rounded to fp32, every product exact in double and
// added in double, wave shuffle, LDS, per-block partials with plain stores, folded by
// sqnorm_fold_kernel. A grid of (blocks, G) would read c and r again for every row, 3 G n words;
// here a thread keeps its quad of d_0 and the two accumulators of a tile of up to RC <= 16 rows in
// registers (as cc_step_kernel keeps its rows), and blockIdx.y walks the tiles of a larger G:
// G + 2 ceil(G / 16) words per coordinate. Tile 0 also forms the root's own squared norm.
// pd / ps: the partials of dots / sq, [G + 1][gridDim.x] each (dots / sq themselves for one block).
constexpr int RD_MAX_ROWS = 16;
constexpr int RD_GRID_CAP = 2048;  // every block ends in up to 33 reductions: few long blocks

template <int RC>
__global__ __launch_bounds__(256) void root_dots_kernel(const float* __restrict__ X, long long ld,
                                                        const float* __restrict__ c, const float* __restrict__ r,
                                                        int G, long long n, double* __restrict__ pd,
                                                        double* __restrict__ ps) {
#pragma clang fp contract(off)
  __shared__ double red[2 * RC + 1][4];
  const bool vec = (ld % 4) == 0 && (((uintptr_t)X | (uintptr_t)c | (uintptr_t)r) & 15) == 0;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  for (int g0 = blockIdx.y * RC; g0 < G; g0 += gridDim.y * RC) {
    const int rows = G - g0 < RC ? G - g0 : RC;  // the same in every thread of the block
    const float* tile = X + (long long)g0 * ld;
    double dot[RC], sq[RC], sq0 = 0.0;
#pragma unroll
    for (int g = 0; g < RC; ++g) dot[g] = sq[g] = 0.0;
    quad_stream(n, vec, [&](long long e, auto w) {
#pragma clang fp contract(off)
      constexpr int W = decltype(w)::value;
      const fvec<W> m = c ? ldv<W>(c + e) : fzero<W>();
      const fvec<W> rt = ldv<W>(r + e);
      fvec<W> x[RC];
#pragma unroll
      for (int g = 0; g < RC; ++g)
        if (g < rows) x[g] = ldv<W>(tile + g * ld + e);
      double d0[W];
#pragma unroll
      for (int i = 0; i < W; ++i) {
        const float d = rt[i] - m[i];
        d0[i] = (double)d;
        sq0 = sq0 + d0[i] * d0[i];
      }
#pragma unroll
      for (int g = 0; g < RC; ++g) {
        if (g >= rows) continue;
#pragma unroll
        for (int i = 0; i < W; ++i) {
          const float d = x[g][i] - m[i];
          dot[g] = dot[g] + (double)d * d0[i];
          sq[g] = sq[g] + (double)d * (double)d;
        }
      }
    });
#pragma unroll
    for (int g = 0; g < RC; ++g) {
      double a = dot[g], b = sq[g];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_xor(a, o, 64);
        b += __shfl_xor(b, o, 64);
      }
      if (lane == 0) {
        red[2 * g][wid] = a;
        red[2 * g + 1][wid] = b;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sq0 += __shfl_xor(sq0, o, 64);
    if (lane == 0) red[2 * RC][wid] = sq0;
    __syncthreads();
    const int t = threadIdx.x;
    if (t < 2 * rows) {
      const double s = (red[t][0] + red[t][1]) + (red[t][2] + red[t][3]);
      ((t & 1) ? ps : pd)[(long long)(g0 + (t >> 1)) * gridDim.x + blockIdx.x] = s;
    } else if (t == 2 * RC && g0 == 0) {
      const double s = (red[t][0] + red[t][1]) + (red[t][2] + red[t][3]);
      pd[(long long)G * gridDim.x + blockIdx.x] = s;
      ps[(long long)G * gridDim.x + blockIdx.x] = s;
    }
    __syncthreads();  // red is reused by the block's next tile
  }
}

static int root_dots_blocks(int G, long long n) {
  const int tiles = (G + RD_MAX_ROWS - 1) / RD_MAX_ROWS;
  const int lim = tiles >= RD_GRID_CAP ? 1 : RD_GRID_CAP / tiles;
  return grid_for((n + 3) / 4, 256, lim);
}

// doubles of scratch `ddl_root_dots` needs for G rows of n coordinates
DDL_API long long ddl_root_dots_workspace(int G, long long n) {
  if (G < 1 || n < 1) return 0;
  return 2LL * (G + 1) * root_dots_blocks(G, n);
}

// dots[G + 1], sq[G + 1] (float64): entry G is the root's own squared norm in both. center == null:
// rows and root already are updates.
DDL_API int ddl_root_dots(const float* X, long long ld, const float* center, const float* root, int G,
                          long long n, double* part, long long part_cap, double* dots, double* sq,
                          hipStream_t s) {
  if (G < 1 || n < 1 || !root || part_cap < ddl_root_dots_workspace(G, n)) return (int)hipErrorInvalidValue;
  const int bx = root_dots_blocks(G, n);
  const int tiles = (G + RD_MAX_ROWS - 1) / RD_MAX_ROWS;
  const int gy = tiles < 65535 ? tiles : 65535;
  // one block: its partials are the results
  double* pd = bx == 1 ? dots : part;
  double* ps = bx == 1 ? sq : part + (long long)(G + 1) * bx;
#define RD_LAUNCH(RC_) \
  hipLaunchKernelGGL((root_dots_kernel<RC_>), dim3(bx, gy), dim3(256), 0, s, X, ld, center, root, G, n, pd, ps)
  if (G <= 4) RD_LAUNCH(4);
  else if (G <= 8) RD_LAUNCH(8);
  else RD_LAUNCH(RD_MAX_ROWS);
#undef RD_LAUNCH
  if (bx > 1) {
    const int gf = G + 1 < 65535 ? G + 1 : 65535;
    hipLaunchKernelGGL(sqnorm_fold_kernel, dim3(gf), dim3(256), 0, s, pd, bx, G + 1, dots);
    hipLaunchKernelGGL(sqnorm_fold_kernel, dim3(gf), dim3(256), 0, s, ps, bx, G + 1, sq);
  }
  return (int)hipGetLastError();
}

// FLTrust's row scales from `ddl_root_dots`' results, one block, double throughout (built like
// gm_scales_kernel): n_k = sqrt(sq_k), n_0 = sqrt(sq[G]); cos_k = clamp(dot_k / (n_k n_0), -1, 1);
// beta_k = coeff_k * max(cos_k, 0); S = beta_0 + beta_1 + ... added by one thread in index order;
// beta_sum[0] = S; cs_k = fl32(beta_k * (n_0 / n_k) / T), T = *total when given (the S of all
// ranks), else S; T == 0 gives cs = 0 throughout. A row is dead when sq_k or dot_k is NaN / Inf or
// n_k == 0, and every row is when sq[G] is NaN / Inf or 0: beta_k = cs_k = 0, cos_k = NaN.
__device__ __forceinline__ bool trust_live(double q, double d, double q0) {
  return q < (double)INFINITY && fabs(d) < (double)INFINITY && q > 0.0 && q0 < (double)INFINITY && q0 > 0.0;
}

__device__ __forceinline__ double trust_cos(double q, double d, double q0) {
  const double cs = d / (sqrt(q) * sqrt(q0));
  return cs < -1.0 ? -1.0 : (cs > 1.0 ? 1.0 : cs);
}

__global__ __launch_bounds__(256) void trust_scales_kernel(const double* __restrict__ dots, const double* __restrict__ sq,
                                                           const float* __restrict__ coeff, int G,
                                                           const double* __restrict__ total, float* __restrict__ cos_out,
                                                           float* __restrict__ norms, float* __restrict__ cs,
                                                           double* __restrict__ beta_sum) {
#pragma clang fp contract(off)
  __shared__ double chunk[256];
  __shared__ double sum;
  const int tid = threadIdx.x;
  const double q0 = sq[G];
  double S = 0.0;
  for (int base = 0; base < G; base += 256) {
    const int k = base + tid;
    if (k < G) {
      const double q = sq[k], d = dots[k];
      norms[k] = (float)sqrt(q);  // +inf for a finite row too long for fp32
      double b = 0.0;
      float co = NAN;
      if (trust_live(q, d, q0)) {
        const double cv = trust_cos(q, d, q0);
        co = (float)cv;
        b = (double)coeff[k] * (cv > 0.0 ? cv : 0.0);
      }
      cos_out[k] = co;
      chunk[tid] = b;
    }
    __syncthreads();
    if (tid == 0) {
      const int m = G - base < 256 ? G - base : 256;
      for (int j = 0; j < m; ++j) S += chunk[j];
    }
    __syncthreads();
  }
  if (tid == 0) {
    beta_sum[0] = S;
    sum = total ? *total : S;
  }
  __syncthreads();
  const double T = sum;
  for (int k = tid; k < G; k += 256) {
    const double q = sq[k], d = dots[k];
    float r = 0.f;
    if (T != 0.0 && trust_live(q, d, q0)) {
      const double cv = trust_cos(q, d, q0);
      const double b = (double)coeff[k] * (cv > 0.0 ? cv : 0.0);
      r = (float)(b * (sqrt(q0) / sqrt(q)) / T);
    }
    cs[k] = r;
  }
}

DDL_API int ddl_trust_scales(const double* dots, const double* sq, const float* coeff, int G, const double* total,
                             float* cos, float* norms, float* cs, double* beta_sum, hipStream_t s) {
  if (G < 1) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(trust_scales_kernel, dim3(1), dim3(256), 0, s, dots, sq, coeff, G, total, cos, norms, cs,
                     beta_sum);
  return (int)hipGetLastError();
}

__global__ void clipped_sum_kernel(const float* __restrict__ X, long long ld, const float* c,
                                   const float* __restrict__ cs, int G, long long n, float* out,
                                   int accumulate) {
  const bool vec = (ld % 4) == 0 && (((uintptr_t)out | (uintptr_t)X | (uintptr_t)c) & 15) == 0;
  quad_stream(n, vec, [&](long long e, auto w) {
    // difference, product and sum each rounded on their own (no fused multiply-add), rows added in
    // order: the same bits wherever the rows live, as weighted_sum_kernel
#pragma clang fp contract(off)
    constexpr int W = decltype(w)::value;
    fvec<W> acc = accumulate ? ldv<W>(out + e) : fzero<W>();
    const fvec<W> m = c ? ldv<W>(c + e) : fzero<W>();
    for (int g = 0; g < G; ++g) {
      const float k = cs[g];
      if (k == 0.f) continue;  // dropped row (or zero weight): not read, 0 * NaN would be NaN
      const fvec<W> v = ldv<W>(X + g * ld + e);
#pragma unroll
      for (int i = 0; i < W; ++i) acc[i] = acc[i] + k * (v[i] - m[i]);
    }
    stv<W>(out + e, acc);
  });
}

DDL_API int ddl_clipped_sum(const float* X, long long ld, const float* center, const float* cs, int G,
                            long long n, float* out, int accumulate, hipStream_t s) {
  if (G < 0 || n < 1) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(clipped_sum_kernel, dim3(grid_for((n + 3) / 4, 256)), dim3(256), 0, s, X, ld,
                     center, cs, G, n, out, accumulate);
  return (int)hipGetLastError();
}

// The robust learning rate (RLR: Ozdayi, Kantarcioglu, Gel, AAAI 2021): a per-coordinate sign vote
// over the client updates, in the same single read of the rows as the clipped sum. With
// u_ki = fl32(x_ki - c_i) over the rows with cs[k] != 0 (the others are not read and do not vote):
//   delta[i] = sum_k cs[k] * u_ki            clipped_sum_kernel's loop: the same order and roundings
//   s_i      = sum_k sgn(u_ki)               sgn(+-0) = sgn(NaN) = 0; unweighted, held as fp32: sums
//                                            of at most G < 2^24 values in {-1, 0, 1}, exact in any order
// theta < 0, the partial mode of several ranks: delta and votes go out as they are (votes required).
// theta >= 0, the final mode: delta[i] is negated where |s_i| < theta, votes written when given.
// Nothing is held per row, so G is bounded by memory only: (G + 2) words per coordinate, one more
// with votes.
__global__ void rlr_sum_kernel(const float* __restrict__ X, long long ld, const float* c,
                               const float* __restrict__ cs, int G, long long n, float theta, float* delta,
                               float* votes) {
  const bool vec = (ld % 4) == 0 &&
                   (((uintptr_t)delta | (uintptr_t)votes | (uintptr_t)X | (uintptr_t)c) & 15) == 0;
  quad_stream(n, vec, [&](long long e, auto w) {
#pragma clang fp contract(off)
    constexpr int W = decltype(w)::value;
    fvec<W> acc = fzero<W>(), s = fzero<W>();
    const fvec<W> m = c ? ldv<W>(c + e) : fzero<W>();
    for (int g = 0; g < G; ++g) {
      const float k = cs[g];
      if (k == 0.f) continue;  // dropped row (or zero weight): not read, no vote
      const fvec<W> v = ldv<W>(X + g * ld + e);
#pragma unroll
      for (int i = 0; i < W; ++i) {
        const float u = v[i] - m[i];
        acc[i] = acc[i] + k * u;
        s[i] = s[i] + (float)((u > 0.f) - (u < 0.f));  // both false for +-0 and NaN
      }
    }
    if (theta >= 0.f) {
#pragma unroll
      for (int i = 0; i < W; ++i)
        if (fabsf(s[i]) < theta) acc[i] = -acc[i];
    }
    stv<W>(delta + e, acc);
    if (votes) stv<W>(votes + e, s);
  });
}

DDL_API int ddl_rlr_sum(const float* X, long long ld, const float* center, const float* cs, int G, long long n,
                        float theta, float* delta, float* votes, hipStream_t s) {
  if (G < 0 || G >= (1 << 24) || n < 1 || !delta || theta != theta || (theta < 0.f && !votes))
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(rlr_sum_kernel, dim3(grid_for((n + 3) / 4, 256)), dim3(256), 0, s, X, ld, center, cs, G,
                     n, theta, delta, votes);
  return (int)hipGetLastError();
}

// delta[i] = -delta[i] where |votes[i]| < theta: the second half of the partial mode, after the
// cross-rank sums of both vectors. Three words per coordinate.
__global__ void rlr_flip_kernel(float* delta, const float* __restrict__ votes, long long n, float theta) {
  const bool vec = (((uintptr_t)delta | (uintptr_t)votes) & 15) == 0;
  quad_stream(n, vec, [&](long long e, auto w) {
    constexpr int W = decltype(w)::value;
    fvec<W> d = ldv<W>(delta + e);
    const fvec<W> s = ldv<W>(votes + e);
#pragma unroll
    for (int i = 0; i < W; ++i)
      if (fabsf(s[i]) < theta) d[i] = -d[i];
    stv<W>(delta + e, d);
  });
}

DDL_API int ddl_rlr_flip(float* delta, const float* votes, long long n, float theta, hipStream_t s) {
  if (n < 1 || !delta || !votes || !(theta >= 0.f)) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(rlr_flip_kernel, dim3(grid_for((n + 3) / 4, 256)), dim3(256), 0, s, delta, votes, n, theta);
  return (int)hipGetLastError();
}

// One iteration of centered clipping (Karimireddy et al. 2021) in ONE read of the rows:
//   v_out[i]   = v_in[i] + sum_k cs[k] * fl32(x_ki - ctr_in[i])   (clipped_sum_kernel's order and
//                roundings, rows with cs[k] == 0 not read)
//   ctr_out[i] = c[i] + v_out[i]                                   (v_out[i] without a centre)
// and, with NORMS, while the row quads are still in registers, the next iteration's squared norms
// part[k][block] = sum_i fl32(x_ki - ctr_out[i])^2 in double: wave shuffle, LDS, plain stores, folded
// by sqnorm_fold_kernel. A row that was not read gets +inf partials: its next cs is 0 again.
// v_out may be v_in and ctr_out may be ctr_in or c: a thread reads its coordinates of every operand
// before it writes them, and no other thread touches those coordinates.
constexpr int CC_MAX_ROWS = 16;
constexpr int CC_GRID_CAP = 2048;  // every block ends in up to 16 reductions: few long blocks

template <int RC, bool NORMS>
__global__ __launch_bounds__(256) void cc_step_kernel(const float* __restrict__ X, long long ld, const float* c,
                                                      const float* ctr_in, const float* v_in,
                                                      const float* __restrict__ cs, int G, long long n,
                                                      float* v_out, float* ctr_out, double* __restrict__ part) {
  __shared__ double red[RC][4];
  const bool vec = (ld % 4) == 0 && (((uintptr_t)X | (uintptr_t)c | (uintptr_t)ctr_in | (uintptr_t)v_in |
                                      (uintptr_t)v_out | (uintptr_t)ctr_out) & 15) == 0;
  float k[RC];
  double sq[RC];
#pragma unroll
  for (int g = 0; g < RC; ++g) {
    k[g] = g < G ? cs[g] : 0.f;
    sq[g] = 0.0;
  }
  quad_stream(n, vec, [&](long long e, auto w) {
#pragma clang fp contract(off)
    constexpr int W = decltype(w)::value;
    fvec<W> acc = ldv<W>(v_in + e);
    const fvec<W> m = ldv<W>(ctr_in + e);
    fvec<W> x[RC];
#pragma unroll
    for (int g = 0; g < RC; ++g) {
      if (k[g] == 0.f) continue;  // dropped row, zero weight or g >= G: not read
      x[g] = ldv<W>(X + g * ld + e);
#pragma unroll
      for (int i = 0; i < W; ++i) acc[i] = acc[i] + k[g] * (x[g][i] - m[i]);
    }
    fvec<W> o = acc;
    if (c) {
      const fvec<W> b = ldv<W>(c + e);
#pragma unroll
      for (int i = 0; i < W; ++i) o[i] = b[i] + acc[i];
    }
    stv<W>(v_out + e, acc);
    stv<W>(ctr_out + e, o);
    if constexpr (NORMS) {
#pragma unroll
      for (int g = 0; g < RC; ++g) {
        if (k[g] == 0.f) continue;
#pragma unroll
        for (int i = 0; i < W; ++i) {
          const float d = x[g][i] - o[i];
          sq[g] = sq[g] + (double)d * (double)d;
        }
      }
    }
  });
  if constexpr (NORMS) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int g = 0; g < RC; ++g) {
      double a = sq[g];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
      if (lane == 0) red[g][wid] = a;
    }
    __syncthreads();
    if (threadIdx.x < RC && (int)threadIdx.x < G) {
      const int g = threadIdx.x;
      const double s = (red[g][0] + red[g][1]) + (red[g][2] + red[g][3]);
      part[(long long)g * gridDim.x + blockIdx.x] = cs[g] == 0.f ? (double)INFINITY : s;
    }
  }
}

// blocks of a `ddl_cc_step` launch: the doubles of scratch it needs per row
DDL_API int ddl_cc_step_blocks(long long n) { return n < 1 ? 0 : grid_for((n + 3) / 4, 256, CC_GRID_CAP); }

// part == null: the last step, no norms. Otherwise sq[G] takes the folded squared norms.
DDL_API int ddl_cc_step(const float* X, long long ld, const float* c, const float* ctr_in, const float* v_in,
                        const float* cs, int G, long long n, float* v_out, float* ctr_out, double* part,
                        long long part_cap, double* sq, hipStream_t s) {
  if (G < 1 || G > CC_MAX_ROWS || n < 1) return (int)hipErrorInvalidValue;
  const int bx = ddl_cc_step_blocks(n);
  if (part && (part_cap < (long long)G * bx || !sq)) return (int)hipErrorInvalidValue;
#define CC_CASE(RC_) \
  if (G <= RC_) { \
    if (part) \
      hipLaunchKernelGGL((cc_step_kernel<RC_, true>), dim3(bx), dim3(256), 0, s, X, ld, c, ctr_in, v_in, cs, G, \
                         n, v_out, ctr_out, part); \
    else \
      hipLaunchKernelGGL((cc_step_kernel<RC_, false>), dim3(bx), dim3(256), 0, s, X, ld, c, ctr_in, v_in, cs, G, \
                         n, v_out, ctr_out, part); \
    if (part) hipLaunchKernelGGL(sqnorm_fold_kernel, dim3(G), dim3(256), 0, s, part, bx, G, sq); \
    return (int)hipGetLastError(); \
  }
  CC_CASE(4) CC_CASE(8) CC_CASE(16)
#undef CC_CASE
  return (int)hipErrorInvalidValue;
}

// Gaussian noise of the server update: z_i is a pure function of (seed, round, global index i).
// Philox key (seed_lo, seed_hi), counter (q_lo, q_hi, TAG, round) with q = i >> 2, and the four
// words r give two Box-Muller pairs: z[4q] = R(r.x) cos(2 pi U(r.y)), z[4q+1] = R(r.x) sin(..),
// z[4q+2] = R(r.z) cos(2 pi U(r.w)), z[4q+3] = R(r.z) sin(..), U = u32_to_unit in (0, 1] and
// R(x) = sqrt(-2 ln U(x)) <= 5.77. The precise logf / sincosf: the pass moves 3n floats, the math
// is free, and the tail of the noise should not depend on an approximate log.
constexpr uint32_t CLIP_NOISE_TAG = 0x3c6ef372u;

__device__ __forceinline__ void normal4(uint2 key, long long q, uint32_t round, float (&z)[4]) {
  const uint4 r = philox4x32(make_uint4((uint32_t)q, (uint32_t)((unsigned long long)q >> 32), CLIP_NOISE_TAG, round), key);
  const float r0 = sqrtf(-2.0f * logf(u32_to_unit(r.x)));
  const float r1 = sqrtf(-2.0f * logf(u32_to_unit(r.z)));
  float s0, c0, s1, c1;
  sincosf(6.2831853071795864769f * u32_to_unit(r.y), &s0, &c0);
  sincosf(6.2831853071795864769f * u32_to_unit(r.w), &s1, &c1);
  z[0] = r0 * c0; z[1] = r0 * s0; z[2] = r1 * c1; z[3] = r1 * s1;
}

// w[j] = (c[j] or 0) + delta[j] + std * z[off + j], j in [0, n). One thread per quad q of the
// GLOBAL index off + j, so a call on a sub-slice draws what the full call draws; `off` need not be a
// multiple of 4 (then the scalar path). w may alias c: every thread reads its elements before it
// writes them. std == 0: exactly c + delta, no RNG work. Not on quad_stream: its quads belong to
// the global index, so the first one may begin before the slice (j0 < 0), which the shared loop
// over [0, n) has no notion of.
__global__ void apply_update_kernel(float* w, const float* c, const float* __restrict__ delta, long long n,
                                    long long off, float std, uint2 key, uint32_t round) {
#pragma clang fp contract(off)
  const long long q0 = off >> 2;
  const long long nq = ((off + n + 3) >> 2) - q0;
  const bool vec = (off & 3) == 0 && (((uintptr_t)w | (uintptr_t)c | (uintptr_t)delta) & 15) == 0;
  for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < nq;
       t += (long long)gridDim.x * blockDim.x) {
    const long long q = q0 + t;
    const long long j0 = q * 4 - off;  // local index of the quad's first element (may be < 0)
    float z[4] = {0.f, 0.f, 0.f, 0.f};
    if (std != 0.f) normal4(key, q, round, z);
    if (vec && j0 + 4 <= n) {
      const float4 d = *(const float4*)(delta + j0);
      float4 o = d;
      if (c) {
        const float4 m = *(const float4*)(c + j0);
        o.x = m.x + d.x; o.y = m.y + d.y; o.z = m.z + d.z; o.w = m.w + d.w;
      }
      if (std != 0.f) {
        o.x = o.x + std * z[0]; o.y = o.y + std * z[1];
        o.z = o.z + std * z[2]; o.w = o.w + std * z[3];
      }
      *(float4*)(w + j0) = o;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const long long j = j0 + e;
        if (j >= 0 && j < n) {
          float o = c ? c[j] + delta[j] : delta[j];
          if (std != 0.f) o = o + std * z[e];
          w[j] = o;
        }
      }
    }
  }
}

DDL_API int ddl_apply_update(float* w, const float* center, const float* delta, long long n, long long off,
                             float std, unsigned long long seed, unsigned int round, hipStream_t s) {
  if (n < 1 || off < 0) return (int)hipErrorInvalidValue;
  const long long nq = ((off + n + 3) >> 2) - (off >> 2);
  hipLaunchKernelGGL(apply_update_kernel, dim3(grid_for(nq, 256)), dim3(256), 0, s, w, center, delta, n,
                     off, std, make_uint2((uint32_t)seed, (uint32_t)(seed >> 32)), (uint32_t)round);
  return (int)hipGetLastError();
}
