// Halo-staged X6 WGRAD of stride-1 "same" 3x3 / 1x1 convolutions (fp32 operands on the bf16 MFMA).
//
// dW[k][r][s][c] = sum over output pixels q of dY[q][k] * X[q + (r - pd, s - pd)][c]. conv_f32.hip
// runs this as an implicit GEMM whose X operand rows are (tap, channel): every X value is loaded,
// split into its three bf16 pieces and transposed into LDS once PER TAP (9x), which makes that loop
// VALU-bound (~6 VALU per MFMA, MFMA busy 30-37 %, profiles/pmc_wgrad_r4.txt). Here a workgroup
// owns dW[k0:k0+64][all taps][c0:c0+32] and sweeps a slice of the pixel tiles; per tile of 64
// output pixels it stages
//   dY  [64 k][64 pixels]                         (planar h | m | l bf16, pixel-contiguous rows)
//   X   [32 c][tile rows + halo][tile cols + halo] (planar, one image row per LDS row)
// each ONCE (register transpose: a thread loads 4 or 8 pixels x 4 channels and writes each channel's
// pixels as one LDS store per plane), and the 9 taps read shifted windows of the X image.
// MFMA v_mfma_f32_32x32x16_bf16 with the REDUCTION over pixels: lane l holds 8 consecutive pixels
// (l >> 5 selects which 8 of the step's 16) of row / column l & 31.
// Per pair of 16-pixel steps and (k block, tap): twelve piece products chained from zero, then ONE
// IEEE add into the fp32 accumulator (the halo FWD / DGRAD kernel's rounding discipline).
//
// 8 waves, two per SIMD, in two roles (DDL_HW_PROBE timings, docs/KERNELS.md: with one wave per
// SIMD doing every phase in turn the phases' times added up):
//   waves 0-3 stage:   they keep the loads of tiles t + 2 and t + 3 in flight (two register sets),
//             split tile t + 1 into its planes and write it to the other LDS stage while tile t's
//             MFMAs run;
//   waves 4-7 compute: wave w owns k block (w >> 1) & 1 (32 rows), all taps, over the even (w even)
//             or odd pixel steps of every tile; they issue only fragment reads, MFMAs and the adds.
// One workgroup barrier per tile hands the two LDS stages over; nothing else is shared, so a launch
// leaves no state behind. The two step-parity halves are summed once at the end.
// Split-K over pixel tiles writes [split][G][K][R*S*C] partial slices for convf32_wgrad_reduce;
// unsplit launches apply out = (accumulate ? out : 0) + gscale * dW directly (direct SGD).
#include <cstdlib>

#include "ddl_common.h"
#include "conv_f32_core.h"

namespace {

typedef float f16v __attribute__((ext_vector_type(16)));  // 32x32 MFMA accumulator

constexpr int HW_BK = 64, HW_BC = 32, HW_TP = 64;  // k rows, channels, pixels per tile
constexpr int HW_KS = 72;    // dY LDS row stride (elements): 144 B = 9 16-byte slots, 32 rows conflict-free
constexpr int HW_NT = 512;   // 4 staging waves + 4 compute waves
constexpr size_t HW_LDS_MAX = 160 * 1024;
constexpr unsigned HW_OOB = 0x80000000u;

struct HWGeo {
  int lgW;      // log2 output width (4..64)
  int SR;       // rows per image segment of a tile (min(64 / OW, OH))
  int NSEG;     // image segments per tile
  int HR, HCp;  // halo rows per segment (SR + R - 1), padded halo row length (elements, % 8 == 0)
  int CS;       // X LDS channel stride (elements)
  int ntile;    // pixel tiles per group
  int probe;    // timing probes (DDL_HW_PROBE, wrong results): 1 skip the split + LDS writes,
                // 2 skip the MFMA loop, 4 skip the global loads (2: staging + loads alone, 5: compute alone)
};

// Prefetch loads in inline asm: the compiler neither sees nor waits on them. hw_wait() at the tile's
// staging is the one wait, and pins every prefetch register behind it. Plain VGPRs: with no AGPR
// constraint in the kernel the compiler keeps the MFMA accumulators in VGPRs too and has all 256
// registers of a wave in one class (an "a" constraint made it halve them 128 / 128 and spill).
typedef int hw_rsrc __attribute__((ext_vector_type(4)));
__device__ __forceinline__ hw_rsrc hw_make_rsrc(const void* p, long long bytes) {
  const unsigned long long a = (unsigned long long)p;
  hw_rsrc r;
  r.x = (int)(unsigned)(a & 0xffffffffull);
  r.y = (int)(unsigned)((a >> 32) & 0xffffull);
  r.z = (int)bytes;
  r.w = 0x00020000;
  return r;
}
__device__ __forceinline__ void hw_load(f4v& d, const hw_rsrc& rs, unsigned off) {
  asm volatile("buffer_load_dwordx4 %0, %1, %2, 0 offen" : "=v"(d) : "v"(off), "s"(rs) : "memory");
}

// 8 values -> the three bf16 planes of one 16-byte LDS row segment each
__device__ __forceinline__ void split8(const float (&v)[8], s8v& h, s8v& m, s8v& l) {
  s4v h0, m0, l0, h1, m1, l1;
  split3(make_float4(v[0], v[1], v[2], v[3]), h0, m0, l0);
  split3(make_float4(v[4], v[5], v[6], v[7]), h1, m1, l1);
  h = cat44(h0, h1);
  m = cat44(m0, m1);
  l = cat44(l0, l1);
}

// A tap's 8-pixel window out of two ALIGNED 16-byte chunks of one plane. Images >= 8 wide: the
// chunks are halo columns pcol .. pcol + 15 of the tap's row, the window starts s elements in.
// 4-wide images (W4): a lane's 8 pixels are two image rows of 4; the chunks are the tap's halo row
// and the one below it (8 elements each), the window is columns s .. s + 3 of both.
template <bool W4>
__device__ __forceinline__ s8v hw_win(const s8v& c0, const s8v& c1, int s) {
  if constexpr (W4) {
    if (s == 0) return __builtin_shufflevector(c0, c1, 0, 1, 2, 3, 8, 9, 10, 11);
    if (s == 1) return __builtin_shufflevector(c0, c1, 1, 2, 3, 4, 9, 10, 11, 12);
    return __builtin_shufflevector(c0, c1, 2, 3, 4, 5, 10, 11, 12, 13);
  } else {
    if (s == 0) return c0;
    if (s == 1) return __builtin_shufflevector(c0, c1, 1, 2, 3, 4, 5, 6, 7, 8);
    return __builtin_shufflevector(c0, c1, 2, 3, 4, 5, 6, 7, 8, 9);
  }
}

template <int RS, bool W4>
__global__ __launch_bounds__(HW_NT) void convx6hw_kernel(ConvF32Args a, HWGeo hg) {
  constexpr int T = RS * RS, PD = (RS - 1) / 2;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int stg = 3 * (HW_BK * HW_KS + HW_BC * hg.CS);      // elements per LDS stage
  bf16_t* const dyl = (bf16_t*)smem;                        // stage b at + b * stg: [3][64][HW_KS]
  bf16_t* const xl = dyl + 3 * HW_BK * HW_KS;               // stage b at + b * stg: [3][32][CS]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);  // scalar: the role branches are uniform
  // staging = the four waves dispatched first: the older wave of a SIMD wins the VALU issue slots, and
  // the staging waves' split is the longer side (measured: +8 % with the compute waves first)
  const bool stager = wid < 4;
  const int ptid = tid & 255;  // index among the staging threads (compute threads: unused)
  const int OW = 1 << hg.lgW, TR = HW_TP >> hg.lgW;
  const int nct = a.C / HW_BC;
  const int k0 = (blockIdx.x / nct) * HW_BK, c0 = (blockIdx.x % nct) * HW_BC;
  const int split = blockIdx.y, nsplit = gridDim.y, g = blockIdx.z;
  // slices are cut in units of two tiles (128 pixels, the tile of the serial kernel this one replaced):
  // the same pixels per slice and so the same summation order, bit for bit, as before the tile halved
  const int per = 2 * (((hg.ntile + 1) / 2 + nsplit - 1) / nsplit);
  const int t0 = split * per, t1 = min(hg.ntile, t0 + per);
  const int K = a.K, C = a.C, H = a.H, W = a.W;
  const long long npix = (long long)a.N * H * W;

  const hw_rsrc rD = hw_make_rsrc(a.dy + (long long)g * a.dy_gs, npix * K * 4);
  const hw_rsrc rX = hw_make_rsrc(a.x + (long long)g * a.x_gs, npix * C * 4);

  const int nt = t1 - t0;  // tiles of this slice; uniform over the workgroup: every wave meets every barrier

  // ---- the tile loop, staging side. LDS stage i & 1 holds tile i of the slice. While the compute
  // waves run tile i the staging waves fill the other stage with tile i + 1 and issue the loads of
  // tile i + 2; the barrier that ends iteration i both publishes stage (i + 1) & 1 and frees
  // stage i & 1. The compute side below meets the same barriers in the same order.
  if (stager) {
    // ---- dY unit: 4 channels k0 + 4 dkc .. + 3 of the tile pixels 4 dpg .. + 3. 16 consecutive
    // lanes hold 4 channel quads x 4 pixel groups: a load instruction reads whole 256-byte runs of
    // channels, and the 8-byte LDS stores of a 16-lane group fall on 8 distinct 8-byte bank pairs
    // (2-way, free) instead of 2 (dkc = lane & 15: 8-way).
    const int dkc = (ptid & 3) | (((ptid >> 4) & 3) << 2), dpg = ((ptid >> 2) & 3) | (((ptid >> 6) & 3) << 2);
    // ---- X unit: 4 channels c0 + 4 ucg .. + 3 of 8 halo columns 8 xc .. + 7 of halo row xrr (over
    // segments; urest = xrr * ncol8 + xc); one unit per staging thread (hw_geo), threads past the
    // image idle. 8 consecutive lanes hold 2 channel quads x 4 consecutive units: their 16-byte LDS
    // stores are 64 contiguous bytes per quad, 64 bytes apart (mod 128) between the quads, so
    // conflict-free (ucg = lane & 7: 4-way, the channel stride is 64 mod 128 bytes).
    const int ucg = (ptid & 1) | (((ptid >> 3) & 3) << 1), urest = ((ptid >> 1) & 3) | (((ptid >> 5) & 7) << 2);
    const int ncol8 = hg.HCp >> 3;
    const bool uvalid = urest < hg.NSEG * hg.HR * ncol8;
    const int uxc = urest % ncol8, xrr = urest / ncol8;
    const int useg = xrr / hg.HR, uhr = xrr - useg * hg.HR;  // halo segment, halo row within it
    const int uoff = 4 * ucg * hg.CS + xrr * hg.HCp + 8 * uxc;  // LDS element offset of the unit's first channel
    // operand-side BN of X (relu(x * scale + shift) on real pixels)
    const bool xf = a.in_scale != nullptr;
    float4 xsc = make_float4(1.f, 1.f, 1.f, 1.f), xsh = make_float4(0.f, 0.f, 0.f, 0.f);
    if (xf && uvalid) {
      const long long cc = (long long)g * C + c0 + 4 * ucg;
      xsc = *(const float4*)(a.in_scale + cc);
      xsh = *(const float4*)(a.in_shift + cc);
    }

    // Two prefetch register sets, so that a tile's loads are issued a whole tile before its split:
    // with one set the loads of tile i + 2 could only be issued after tile i + 1 was split, and their
    // latency came on top of every tile's staging (the staging waves are this kernel's critical path).
    struct Regs {
      f4v d[4], x[8];
      unsigned ok;  // bit j: halo pixel j of the unit is a real input pixel
    };
    constexpr int NLD = 12;  // loads per set
    // Every tile index is loaded, past the slice and past the image too (out-of-range pixels read 0
    // through the buffer descriptors): the counted wait below then holds for every tile.
    auto load_tile = [&](int tile, Regs& q) {
      if (hg.probe & 4) return;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const long long p = (long long)tile * HW_TP + dpg * 4 + j;
        hw_load(q.d[j], rD, p < npix ? (unsigned)(((int)p * K + k0 + 4 * dkc) * 4) : HW_OOB);
      }
      // first output row of the tile over (n, oh): tile rows are whole image rows, one (uniform)
      // division per tile; a segment past the first is a whole image (seg * SR == seg * P)
      const int row0 = tile * TR;
      const int n0 = row0 / a.P, oh0 = row0 - n0 * a.P;
      const int n = n0 + useg;
      const int ih = oh0 + uhr - PD;
      q.ok = 0;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int iw = 8 * uxc + j - PD;
        const bool ok = uvalid && n < a.N && (unsigned)ih < (unsigned)H && (unsigned)iw < (unsigned)W;
        q.ok |= (ok ? 1u : 0u) << j;
        hw_load(q.x[j], rX, ok ? (unsigned)((((n * H + ih) * W + iw) * C + c0 + 4 * ucg) * 4) : HW_OOB);
      }
    };
    // wait for set q, the OLDER of the two sets in flight (loads return in order)
    auto hw_wait = [&](Regs& q) {
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NLD) : "memory");
#pragma unroll
      for (int j = 0; j < 4; ++j) asm volatile("" : "+v"(q.d[j]));
#pragma unroll
      for (int j = 0; j < 8; ++j) asm volatile("" : "+v"(q.x[j]));
    };
    // split the loaded tile into its bf16 planes and write them to LDS stage b. This runs in the
    // staging waves only: splitting the next tile inside the compute waves (between the two halves of
    // the current one) was measured 5 % slower, the extra live registers pushed the accumulators
    // through AGPR moves (docs/KERNELS.md).
    auto write_tile = [&](int b, const Regs& q) {
      if (hg.probe & 1) return;
      bf16_t* const dys = dyl + b * stg;
      bf16_t* const xs = xl + b * stg;
      // dY: channel ch of the unit -> row k = 4 dkc + ch, pixels 4 dpg .. + 3
#pragma unroll
      for (int ch = 0; ch < 4; ++ch) {
        float4 v;
        v.x = ch == 0 ? q.d[0].x : ch == 1 ? q.d[0].y : ch == 2 ? q.d[0].z : q.d[0].w;
        v.y = ch == 0 ? q.d[1].x : ch == 1 ? q.d[1].y : ch == 2 ? q.d[1].z : q.d[1].w;
        v.z = ch == 0 ? q.d[2].x : ch == 1 ? q.d[2].y : ch == 2 ? q.d[2].z : q.d[2].w;
        v.w = ch == 0 ? q.d[3].x : ch == 1 ? q.d[3].y : ch == 2 ? q.d[3].z : q.d[3].w;
        s4v h, m, l;
        split3(v, h, m, l);
        bf16_t* d = dys + (4 * dkc + ch) * HW_KS + 4 * dpg;
        *(s4v*)d = h;
        *(s4v*)(d + HW_BK * HW_KS) = m;
        *(s4v*)(d + 2 * HW_BK * HW_KS) = l;
      }
      if (!uvalid) return;
#pragma unroll
      for (int ch = 0; ch < 4; ++ch) {
        const float sc = ch == 0 ? xsc.x : ch == 1 ? xsc.y : ch == 2 ? xsc.z : xsc.w;
        const float sh = ch == 0 ? xsh.x : ch == 1 ? xsh.y : ch == 2 ? xsh.z : xsh.w;
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float e = ch == 0 ? q.x[j].x : ch == 1 ? q.x[j].y : ch == 2 ? q.x[j].z : q.x[j].w;
          if (xf && ((q.ok >> j) & 1u)) {
            e = e * sc + sh;
            if (a.in_relu) e = fmaxf(e, 0.f);
          }
          v[j] = e;
        }
        s8v h, m, l;
        split8(v, h, m, l);
        bf16_t* d = xs + uoff + ch * hg.CS;
        *(s8v*)d = h;
        *(s8v*)(d + HW_BC * hg.CS) = m;
        *(s8v*)(d + 2 * HW_BC * hg.CS) = l;
      }
    };
    if (nt > 0) {
      Regs qa, qb;  // qa: even tiles of the slice, qb: odd tiles
      load_tile(t0, qa);
      load_tile(t0 + 1, qb);
      hw_wait(qa);
      write_tile(0, qa);
      load_tile(t0 + 2, qa);
      __syncthreads();
      // iteration i: stage tile i + 1 out of its set, then refill the set with tile i + 3
      auto step = [&](int i, Regs& q) {
        if (i + 1 < nt) {
          hw_wait(q);
          write_tile((i + 1) & 1, q);
          load_tile(t0 + i + 3, q);
        }
        __syncthreads();
      };
      for (int i = 0; i < nt; i += 2) {
        step(i, qb);
        if (i + 1 < nt) step(i + 1, qa);
      }
    }
    __syncthreads();  // the two barriers of the compute waves' final sum
    __syncthreads();
    return;
  }

  // ---- fragments: compute wave (kb, kh): k block kb (32 rows), the steps ks = kh, kh + 2 of each
  // tile, ALL taps. lane l: row / column l & 31, pixels 8 (l >> 5) .. + 7. A tap's window is read as
  // 16-byte-ALIGNED chunks per plane and shifted out of those registers (hw_win; misaligned
  // ds_read_b128 run at a fraction of the LDS rate: profiles/x6hw_wgrad_r4.txt). One chain at a
  // time: a single chain of this MFMA issues back to back, and three interleaved chains would not
  // fit the 256 registers a wave has at two waves per SIMD beside the 9 x 16 accumulators.
  const int kb = (wid >> 1) & 1, kh = wid & 1;
  int ao[2], xb[2];  // the wave's two steps: dY fragment offset, halo offset of the first pixel (tap (0, 0))
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int ks = 2 * j + kh;
    const int p = 16 * ks + 8 * (lane >> 5);
    const int prow = p >> hg.lgW, pcol = p & (OW - 1);
    const int seg = prow / hg.SR, r = prow - seg * hg.SR;
    ao[j] = (kb * 32 + (lane & 31)) * HW_KS + p;
    xb[j] = (lane & 31) * hg.CS + (seg * hg.HR + r) * hg.HCp + pcol;
  }
  const int c1o = W4 ? hg.HCp : 8;  // second chunk: the halo row below (W4) or the next 8 columns
  f16v acc[T];
#pragma unroll
  for (int t = 0; t < T; ++t)
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[t][v] = 0.f;

  auto compute_tile = [&](int b) {
    const bf16_t* const dys = dyl + b * stg;
    const bf16_t* const xs = xl + b * stg;
    // two own steps per chain: twelve piece products from zero, then one IEEE add per tap
    s8v ah[2], am[2], al[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const bf16_t* ap = dys + ao[j];
      ah[j] = *(const s8v*)ap;
      am[j] = *(const s8v*)(ap + HW_BK * HW_KS);
      al[j] = *(const s8v*)(ap + 2 * HW_BK * HW_KS);
    }
#pragma unroll
    for (int r = 0; r < RS; ++r) {
#pragma unroll
      for (int s2 = 0; s2 < RS; ++s2) {
        f16v c;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const bf16_t* bp = xs + xb[j] + r * hg.HCp;
          const s8v h0 = *(const s8v*)bp, m0 = *(const s8v*)(bp + HW_BC * hg.CS),
                    l0 = *(const s8v*)(bp + 2 * HW_BC * hg.CS);
          s8v h1 = h0, m1 = m0, l1 = l0;
          if (W4 || s2 > 0) {
            h1 = *(const s8v*)(bp + c1o);
            m1 = *(const s8v*)(bp + c1o + HW_BC * hg.CS);
            l1 = *(const s8v*)(bp + c1o + 2 * HW_BC * hg.CS);
          }
          const s8v bh = hw_win<W4>(h0, h1, s2), bm = hw_win<W4>(m0, m1, s2), bl = hw_win<W4>(l0, l1, s2);
          c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[j], bh, j ? c : (f16v){}, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[j], bl, c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am[j], bm, c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[j], bm, c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am[j], bh, c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[j], bh, c, 0, 0, 0);
        }
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[r * RS + s2][v] = acc[r * RS + s2][v] + c[v];
      }
    }
  };

  // ---- the tile loop, compute side
  if (nt > 0) {
    __syncthreads();
    for (int i = 0; i < nt; ++i) {
      if (!(hg.probe & 2)) compute_tile(i & 1);
      __syncthreads();
    }
  }

  // ---- the two step-parity halves of each k block: kh = 1 hands its sums to kh = 0 through LDS
  // (fixed order: deterministic), which adds and writes
  __syncthreads();
  float* const red = (float*)smem;  // [2 kb][T][16][64]
  if (kh == 1) {
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
      for (int v = 0; v < 16; ++v) red[((kb * T + t) * 16 + v) * 64 + lane] = acc[t][v];
  }
  __syncthreads();
  if (kh == 1) return;
  // the other half's sums are added tap by tap inside the epilogue: all 144 LDS reads issued ahead
  // of the adds do not fit beside the accumulators (sched_barrier: the scheduler hoists them)
  auto tap_sum = [&](int t) {
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[t][v] = acc[t][v] + red[((kb * T + t) * 16 + v) * 64 + lane];
  };

  // ---- epilogue: 32x32 block (kb, tap): col = lane & 31 (channel), row = 8 (v >> 2) + 4 (lane >> 5) + (v & 3).
  // Every address is a wave-uniform pointer (slice, k block, tap, register: scalar registers) plus
  // one per-lane 32-bit byte offset: 144 per-lane 64-bit addresses beside the accumulators do not
  // fit a wave's 256 registers. The three store forms are uniform branches.
  const int qd = T * C;  // dW row length (taps x channels); K * qd * 4 < 2^31 (hw_geo)
  const bool split_store = nsplit > 1;
  float* const dst = (split_store ? a.partial + ((long long)split * a.G + g) * K * qd : a.out + (long long)g * a.out_gs) +
                     (long long)(k0 + kb * 32) * qd + c0;
  const unsigned loff = (unsigned)((4 * (lane >> 5) * qd + (lane & 31)) * 4);  // bytes
  auto eptr = [&](int t, int v) { return (float*)((char*)(dst + (8 * (v >> 2) + (v & 3)) * qd + t * C) + loff); };
  if (split_store) {
#pragma unroll
    for (int t = 0; t < T; ++t) {
      tap_sum(t);
#pragma unroll
      for (int v = 0; v < 16; ++v) *eptr(t, v) = acc[t][v];
    }
  } else if (a.accumulate) {
#pragma unroll
    for (int t = 0; t < T; ++t) {
      // the read-modify-write's 16 loads are all issued before the first use (one at a time, each
      // waited out, they serialised the unsplit epilogue)
      tap_sum(t);
      float old[16];
#pragma unroll
      for (int v = 0; v < 16; ++v) old[v] = *eptr(t, v);
#pragma unroll
      for (int v = 0; v < 16; ++v) *eptr(t, v) = old[v] + a.gscale * acc[t][v];
    }
  } else {
#pragma unroll
    for (int t = 0; t < T; ++t) {
      tap_sum(t);
#pragma unroll
      for (int v = 0; v < 16; ++v) *eptr(t, v) = 0.f + a.gscale * acc[t][v];
    }
  }
}

}  // namespace

static bool hw_geo(const ConvF32Args& a, HWGeo& h, int& rs) {
  if (a.stride != 1 || a.R != a.S || (a.R != 1 && a.R != 3) || a.pad != (a.R - 1) / 2) return false;
  if (a.P != a.H || a.Q != a.W || a.K % HW_BK || a.C % HW_BC) return false;
  const int OW = a.Q, OH = a.P;
  if (OW < 4 || OW > HW_TP || (OW & (OW - 1))) return false;
  rs = a.R;
  int lg = 0;
  while ((1 << lg) < OW) ++lg;
  const int TR = HW_TP / OW;
  int SR;
  if (TR <= OH) {
    if (OH % TR) return false;
    SR = TR;
  } else {
    if (TR % OH) return false;
    SR = OH;
  }
  if (OW == 4 && (SR & 1)) return false;  // a lane's 8 pixels are two rows of one image
  h.lgW = lg;
  h.SR = SR;
  h.NSEG = TR / SR;
  h.HR = SR + a.R - 1;
  h.HCp = (OW + a.S - 1 + 7) / 8 * 8;
  const int img = h.NSEG * h.HR * h.HCp;
  h.CS = (img - 8 + 127) / 128 * 128 + 8;  // >= img, == 8 (mod 128): 16 B apart mod 256 B per channel
  const long long npix = (long long)a.N * a.P * a.Q;
  h.ntile = (int)((npix + HW_TP - 1) / HW_TP);
  const int nxu = 8 * h.NSEG * h.HR * (h.HCp / 8);
  if (nxu > 256) return false;  // one X unit per staging thread
  static const int probe = getenv("DDL_HW_PROBE") ? atoi(getenv("DDL_HW_PROBE")) : 0;
  h.probe = probe;
  const long long lim = (1LL << 31) - 64;
  if (npix * a.C * 4 > lim || npix * a.K * 4 > lim) return false;
  if ((long long)a.K * a.R * a.S * a.C * 4 > lim) return false;  // the epilogue's 32-bit dW offsets
  return true;
}

static size_t hw_lds(const HWGeo& h, int T) {
  const size_t stages = (size_t)2 * 3 * (HW_BK * HW_KS + HW_BC * h.CS) * 2;  // two stages of bf16 planes
  const size_t red = (size_t)2 * T * 16 * 64 * 4;  // the epilogue's cross-wave sums
  return stages > red ? stages : red;
}

extern "C" __attribute__((visibility("default"))) int ddl_x6hw_ok(const ConvF32Args* ap) {
  HWGeo h;
  int rs;
  return hw_geo(*ap, h, rs) && hw_lds(h, rs * rs) <= HW_LDS_MAX ? 1 : 0;
}

// the split-K planner's units per group: pairs of pixel tiles (128 pixels), which is how the kernel cuts slices
extern "C" __attribute__((visibility("default"))) int ddl_x6hw_tiles(const ConvF32Args* ap) {
  HWGeo h;
  int rs;
  return hw_geo(*ap, h, rs) ? (h.ntile + 1) / 2 : 0;
}

template <int RS, bool W4>
static int launch_hw(const ConvF32Args& a, const HWGeo& h, hipStream_t s) {
  const int split = a.split_k < 1 ? 1 : a.split_k;
  const size_t lds = hw_lds(h, RS * RS);
  static bool attr_set = false;
  if (!attr_set) {
    hipFuncSetAttribute((const void*)convx6hw_kernel<RS, W4>, hipFuncAttributeMaxDynamicSharedMemorySize,
                        (int)HW_LDS_MAX);
    attr_set = true;
  }
  const dim3 grid((unsigned)((a.K / HW_BK) * (a.C / HW_BC)), (unsigned)split, (unsigned)a.G);
  hipLaunchKernelGGL((convx6hw_kernel<RS, W4>), grid, dim3(HW_NT), lds, s, a, h);
  return (int)hipGetLastError();
}

extern "C" __attribute__((visibility("default"))) int ddl_x6hw(const ConvF32Args* ap, hipStream_t s) {
  const ConvF32Args& a = *ap;
  HWGeo h;
  int rs;
  if (a.G < 1 || a.N < 1 || !hw_geo(a, h, rs) || hw_lds(h, rs * rs) > HW_LDS_MAX) return (int)hipErrorInvalidValue;
  const int split = a.split_k < 1 ? 1 : a.split_k;
  if (split > 1) {
    const long long need = (long long)split * a.G * a.K * a.R * a.S * a.C;
    if (!a.partial || need > a.partial_cap) return (int)hipErrorInvalidValue;
  }
  if (rs == 3) return h.lgW == 2 ? launch_hw<3, true>(a, h, s) : launch_hw<3, false>(a, h, s);
  return h.lgW == 2 ? launch_hw<1, true>(a, h, s) : launch_hw<1, false>(a, h, s);
}
