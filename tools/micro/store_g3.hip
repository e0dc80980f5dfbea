// Diagnostic micro-benchmark (round 6, not part of the product): HBM write rate of stage A's drain in the two plane forms of G.
// Rows of 40192 B (plane form 1) / 53376 B (plane form 0), 44440 rows x 2 slices; a wave covers 4 product blocks (16 G columns) of 32-row
// tiles, a workgroup 512 rows, as ddp_stage_a_h2_kernel<60, GH> does.   hipcc --offload-arch=gfx950 -O3 -o tools/micro/store_g3 tools/micro/store_g3.hip
//   F0  form 0 as shipped: per block and half tile a 16-row x 64-B hi store and a 16-row x 64-B lo store that interleave into whole 128-B lines
//   G0  form 1 as first built: per block and half tile a 16-row x 64-B hi store (dwordx4) and a 16-row x 32-B lo store (dwordx2), hi and lo regions apart
//   G1  ... the lo store as dwordx4 from every second lane (pairs of columns)
//   G2  ... the stores of a row tile's 4 blocks grouped: 8 hi stores back to back, then 8 lo stores (what registers would have to hold)
//   G3  ... lo pieces padded to 16 B (no byte saving: is it the 32-B segment?)
//   G4  G0 with non-temporal stores
//   H0  24-byte units (hi 16 B + lo 8 B side by side: a wave's 16 units = 384 contiguous bytes per row): dwordx4 + dwordx2 per block and half tile
//   H1  ... as 12-byte pieces (4 values: 4 fp16 + 4 bytes), one dwordx3 store per lane, 8 rows x 96 B per instruction, 4 per block
//   H2  H1 with the 4 blocks of a row group back to back (what holding a row tile's four blocks would allow)
//   D0  3 MFMA waves with the kernel's arithmetic + 1 store wave that also splits x (below: "D modes"; `store_g3 dw` runs these alone)
//   D1  ... the x split on the MFMA waves: the store wave issues no loads
//   Every F / G / H mode also with the stores spaced as in the kernel (SL > 0: s_sleep behind every store instruction, two workgroups per CU through LDS)
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <type_traits>
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)
constexpr int NROWS = 44440, NZ = 2, N8 = 23, GCP = 72;
constexpr int LD0 = 13344, LD1 = 10048;     // floats per row

// a wave's 16 G columns at k8 group `g8`: byte offsets inside a row.  Parts are ignored (one tile of GCP columns): the access shape is the same
typedef float f32x3 __attribute__((ext_vector_type(3)));
template <int MODE, int SL = 0>
__global__ __launch_bounds__(256) void drain(float* out, int mrows) {
  extern __shared__ float dyn_lds[];
  if (mrows < 0) dyn_lds[threadIdx.x] = 0.f;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int unit0 = ((int)blockIdx.x * 4 + wave) * 16;       // first (k8, c) unit of the wave: 16 consecutive units
  if (unit0 >= N8 * GCP) return;
  const int ld = (MODE == 0 || MODE == 4) ? LD0 : LD1;
  char* ob = reinterpret_cast<char*>(out) + (size_t)blockIdx.z * NROWS * ld * 4;
  const int R0 = (int)blockIdx.y * mrows, R1 = min(NROWS, R0 + mrows);
  const f32x4 v = {1.f, 2.f, 3.f, (float)lane};
  const f32x2 v2 = {1.f, (float)lane};
  const int g = lane & 3;
  for (int row0 = R0; row0 < R1; row0 += 32) {
    if (MODE == 3) {        // grouped: all hi stores of the row tile, then all lo stores
      for (int t = 0; t < 4; ++t)
        for (int h = 0; h < 2; ++h) {
          const int rr = min(row0 + 16 * h + (lane >> 2), R1 - 1), u = unit0 + 4 * t + g;
          *reinterpret_cast<f32x4*>(ob + (size_t)rr * ld * 4 + (size_t)u * 16) = v;
        }
      for (int t = 0; t < 4; ++t)
        for (int h = 0; h < 2; ++h) {
          const int rr = min(row0 + 16 * h + (lane >> 2), R1 - 1), u = unit0 + 4 * t + g;
          *reinterpret_cast<f32x2*>(ob + (size_t)rr * ld * 4 + (size_t)N8 * GCP * 16 + (size_t)u * 8) = v2;
        }
      continue;
    }
    if (MODE == 7 || MODE == 8) {      // 12-byte pieces: lane (row 8 p + lane / 8, piece lane % 8) of quarter p of block t
      const f32x3 v3 = {1.f, 2.f, (float)lane};
      if (MODE == 7) {
        for (int t = 0; t < 4; ++t)
          for (int p = 0; p < 4; ++p) {
            const int rr = min(row0 + 8 * p + (lane >> 3), R1 - 1);
            *reinterpret_cast<f32x3*>(ob + (size_t)rr * ld * 4 + (size_t)(unit0 + 4 * t) * 24 + 12 * (lane & 7)) = v3;
            if (SL) __builtin_amdgcn_s_sleep(SL);
          }
      } else {
        for (int p = 0; p < 4; ++p)
          for (int t = 0; t < 4; ++t) {
            const int rr = min(row0 + 8 * p + (lane >> 3), R1 - 1);
            *reinterpret_cast<f32x3*>(ob + (size_t)rr * ld * 4 + (size_t)(unit0 + 4 * t) * 24 + 12 * (lane & 7)) = v3;
            if (SL) __builtin_amdgcn_s_sleep(SL);
          }
      }
      continue;
    }
    for (int t = 0; t < 4; ++t)
      for (int h = 0; h < 2; ++h) {
        const int rr = min(row0 + 16 * h + (lane >> 2), R1 - 1), u = unit0 + 4 * t + g;
        char* rowp = ob + (size_t)rr * ld * 4;
        if (MODE == 6) {
          *reinterpret_cast<f32x4*>(rowp + (size_t)u * 24) = v;
          if (SL) __builtin_amdgcn_s_sleep(SL);
          *reinterpret_cast<f32x2*>(rowp + (size_t)u * 24 + 16) = v2;
          if (SL) __builtin_amdgcn_s_sleep(SL);
        } else if (MODE == 0) {
          *reinterpret_cast<f32x4*>(rowp + (size_t)u * 32) = v;
          if (SL) __builtin_amdgcn_s_sleep(SL);
          *reinterpret_cast<f32x4*>(rowp + (size_t)u * 32 + 16) = v;
          if (SL) __builtin_amdgcn_s_sleep(SL);
        } else if (MODE == 1) {
          *reinterpret_cast<f32x4*>(rowp + (size_t)u * 16) = v;
          if (SL) __builtin_amdgcn_s_sleep(SL);
          *reinterpret_cast<f32x2*>(rowp + (size_t)N8 * GCP * 16 + (size_t)u * 8) = v2;
          if (SL) __builtin_amdgcn_s_sleep(SL);
        } else if (MODE == 2) {
          *reinterpret_cast<f32x4*>(rowp + (size_t)u * 16) = v;
          if ((lane & 1) == 0) *reinterpret_cast<f32x4*>(rowp + (size_t)N8 * GCP * 16 + (size_t)u * 8) = v;
        } else if (MODE == 4) {   // lo padded to 16 B: a second full-size region (the row is longer: reads LD0-sized rows)
          *reinterpret_cast<f32x4*>(rowp + (size_t)u * 16) = v;
          *reinterpret_cast<f32x4*>(rowp + (size_t)N8 * GCP * 16 + (size_t)u * 16) = v;
        } else if (MODE == 5) {
          __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(rowp + (size_t)u * 16));
          __builtin_nontemporal_store(v2, reinterpret_cast<f32x2*>(rowp + (size_t)N8 * GCP * 16 + (size_t)u * 8));
        }
      }
  }
}

// ---- D modes: the drain handed to a STORE WAVE, with the kernel's own instruction mix beside it (tools/micro/store_g3 dw).
// A workgroup of 3 MFMA waves + 1 store wave covers 384 product columns = twelve 32-column blocks = THREE 384-byte row groups of the
// 24-byte units.  MFMA wave w computes block 3 j + w in round j = 0 .. 3 of a 32-row tile (12 v_mfma_f32_32x32x16_f16 on weights held in
// registers, then the 19-bit conversion of its four accumulator quads into the group's image in LDS: what block3 of ddp_stage_a_h2_kernel
// does); group g = blocks 4 g .. 4 g + 3 is complete behind round g + 1.  One bare barrier (lgkmcnt(0) in front) ends every round; the store
// wave copies group g out in round g + 2 (twelve 16-byte stores of whole lines, drain3's shape) and in round 1, where no group is due,
// splits the NEXT tile of x into its fp16 planes (PARKD; otherwise the MFMA waves do that behind round 3).  Three images of 12.25 KB + the
// 18 KB of x = 54.75 KB of LDS, two workgroups per CU.  (4 MFMA waves + 1 store wave is not admissible with the weights in registers: ten
// waves on a CU's four SIMDs put three on one, 168 registers each, and the weights, the operand fragments and one accumulator are 176.)
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
constexpr int DW_NG = 105, DW_LD = 96 * DW_NG, DW_NCOLS = 128 * DW_NG, DW_LDX = 180, DW_NPL = 23 * 72;   // the layer-3 G row: 40320 B
#define DW_BAR()                                      \
  do {                                                \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); \
    __builtin_amdgcn_s_barrier();                     \
    asm volatile("" ::: "memory");                    \
  } while (0)
template <bool PARKD>
__global__ __launch_bounds__(256, 2) void drainwave(const float* __restrict__ x, const _Float16* __restrict__ wh, float* __restrict__ out, int nrows,
                                                    int mrows, int* flag) {
  constexpr int KT = 60, KP = 64, NS = 4, XS = KP + 8, RS3 = 392;
  __shared__ __attribute__((aligned(16))) _Float16 xt[2][2][32 * XS];
  __shared__ __attribute__((aligned(16))) char img[3][32 * RS3];
  const int z = (int)blockIdx.z, tid = (int)threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, r = lane & 31, hh = lane >> 5;
  const int colw = (int)blockIdx.x * 384;
  const int ngr = min(3, (DW_NCOLS - colw) / 128);
  const int R0 = (int)blockIdx.y * mrows, R1 = min(nrows, R0 + mrows);
  if (R0 >= nrows) return;
  const float* __restrict__ xb = x + 60 * z;
  for (int i = tid; i < 2 * 2 * 32 * (KP - KT); i += 256) {
    const int kk = i % (KP - KT), rr = (i / (KP - KT)) % 32, bp = i / ((KP - KT) * 32);
    xt[bp / 2][bp % 2][rr * XS + KT + kk] = (_Float16)0.f;
  }
  constexpr int NP = 32 * (KT / 4);                 // 16-byte pieces of an x tile
  auto split = [&](const f32x4 v, int i, int buf) {
    const int rr = i / (KT / 4), q = i % (KT / 4);
    h4 h, l;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float f = v[e] * 2.f;
      if (!(fabsf(f) <= 65504.f)) *flag = 1;
      h[e] = (_Float16)f;
      l[e] = (_Float16)(f - (float)h[e]);
    }
    *reinterpret_cast<h4*>(&xt[buf][0][rr * XS + 4 * q]) = h;
    *reinterpret_cast<h4*>(&xt[buf][1][rr * XS + 4 * q]) = l;
  };
  if (wave == 3) {
    // ---- the store wave
    constexpr int NV = (NP + 63) / 64;
    f32x4 xv[NV];
    auto fetch = [&](int row0) {
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        const int i = lane + 64 * v;
        const int ri = min(row0 + min(i / (KT / 4), 31), nrows - 1);
        xv[v] = *reinterpret_cast<const f32x4*>(xb + (size_t)ri * DW_LDX + 4 * (i % (KT / 4)));
      }
    };
    auto park = [&](int buf) {
#pragma unroll
      for (int v = 0; v < NV; ++v)
        if (lane + 64 * v < NP) split(xv[v], lane + 64 * v, PARKD ? buf : 0);
    };
    int dl[12];
    size_t doff[12];
    float* __restrict__ ob = out + (size_t)z * nrows * DW_LD + 6 * (colw >> 3);
    auto drain = [&](int g) {
      const char* im = img[g];
      float* __restrict__ og = ob + 96 * g;
#pragma unroll
      for (int k = 0; k < 12; ++k) {
        const u32x2 lo8 = *reinterpret_cast<const u32x2*>(im + dl[k]);
        const u32x2 hi8 = *reinterpret_cast<const u32x2*>(im + dl[k] + 8);
        *reinterpret_cast<u32x4*>(og + doff[k]) = u32x4{lo8[0], lo8[1], hi8[0], hi8[1]};
      }
    };
    // (the number of groups is a compile-time constant of the loop: hipcc then counts the stores behind the x loads exactly, and the
    // wait in front of the split is vmcnt(36 + ...), not a drain of the store queue)
    auto run = [&](auto ngr_tag) {
      constexpr int NGR = decltype(ngr_tag)::value;
      if (PARKD) {
        fetch(R0);
        park(0);
        fetch(R0 + 32);
      }
      DW_BAR();
      int n = 0;
      for (int row0 = R0; row0 < R1; row0 += 32, ++n) {
        const int buf = n & 1;
        if (n > 0 && NGR > 2) drain(2);                 // round 0: the previous tile's last group
        DW_BAR();
        {                                               // round 1: this tile's store addresses, the next tile of x
          const int nr = R1 - row0, rid = min(row0 + r, nrows - 1);
#pragma unroll
          for (int k = 0; k < 12; ++k) {
            const int i = 64 * (k % 3) + lane, rl = min(8 * (k / 3) + i / 24, nr - 1);
            dl[k] = rl * RS3 + 16 * (i % 24);
            doff[k] = (size_t)__shfl(rid, rl) * DW_LD + 4 * (i % 24);
          }
          if (PARKD) {
            if (row0 + 32 < R1) park(buf ^ 1);
            fetch(row0 + 64);
          }
        }
        DW_BAR();
        drain(0);                                       // round 2
        DW_BAR();
        if (NGR > 1) drain(1);                          // round 3
        DW_BAR();
      }
      if (NGR > 2) drain(2);
    };
    if (ngr == 3)
      run(std::integral_constant<int, 3>{});
    else if (ngr == 2)
      run(std::integral_constant<int, 2>{});
    else
      run(std::integral_constant<int, 1>{});
    return;
  }
  // ---- an MFMA wave: blocks 3 j + wave
  h8 wr[4][2][NS];
  unsigned sp = 0u;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int c0 = colw + 32 * (3 * j + wave), c = min(c0 + r, DW_NCOLS - 1);
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int s2 = 0; s2 < NS; ++s2) wr[j][p][s2] = *reinterpret_cast<const h8*>(wh + (((((size_t)z * 2 + p) * NS + s2) * 2 + hh) * DW_NCOLS + c) * 8);
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if ((c0 >> 3) + q < DW_NPL) sp |= 1u << (4 * j + q);
  }
  float gh_max = 0.f;
  constexpr int NVM = (NP + 191) / 192;
  f32x4 xm[NVM];
  auto fetch_m = [&](int row0) {
#pragma unroll
    for (int v = 0; v < NVM; ++v) {
      const int i = min(tid + 192 * v, NP - 1);
      const int ri = min(row0 + i / (KT / 4), nrows - 1);
      xm[v] = *reinterpret_cast<const f32x4*>(xb + (size_t)ri * DW_LDX + 4 * (i % (KT / 4)));
    }
  };
  auto park_m = [&](int buf) {
#pragma unroll
    for (int v = 0; v < NVM; ++v)
      if (tid + 192 * v < NP) split(xm[v], tid + 192 * v, buf);
  };
  if (!PARKD) {
    fetch_m(R0);
    park_m(0);
  }
  DW_BAR();
  int n = 0;
  for (int row0 = R0; row0 < R1; row0 += 32, ++n) {
    const int buf = n & 1;
    const bool more = row0 + 32 < R1;
    if (!PARKD && more) fetch_m(row0 + 32);
    h8 a[2][NS];
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int s2 = 0; s2 < NS; ++s2) a[p][s2] = *reinterpret_cast<const h8*>(&xt[buf][p][r * XS + 16 * s2 + 8 * hh]);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int b = 3 * j + wave;
      if ((b >> 2) < ngr) {
        f32x16 am;
#pragma unroll
        for (int i = 0; i < 16; ++i) am[i] = 0.f;
#pragma unroll
        for (int s2 = 0; s2 < NS; ++s2) {
          am = __builtin_amdgcn_mfma_f32_32x32x16_f16(wr[j][0][s2], a[0][s2], am, 0, 0, 0);
          am = __builtin_amdgcn_mfma_f32_32x32x16_f16(wr[j][1][s2], a[0][s2], am, 0, 0, 0);
          am = __builtin_amdgcn_mfma_f32_32x32x16_f16(wr[j][0][s2], a[1][s2], am, 0, 0, 0);
        }
        char* tl = img[b >> 2] + r * RS3 + 96 * (b & 3);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const bool s = ((sp >> (4 * j + q)) & 1u) != 0u;
          const float v0 = am[4 * q], v1 = am[4 * q + 1], v2 = am[4 * q + 2], v3 = am[4 * q + 3];
          gh_max = fmaxf(gh_max, s ? fmaxf(fmaxf(fabsf(v0), fabsf(v1)), fmaxf(fabsf(v2), fabsf(v3))) : 0.f);
          const uint32_t b0 = __builtin_bit_cast(uint32_t, v0) + 0x10u, b1 = __builtin_bit_cast(uint32_t, v1) + 0x10u;
          const uint32_t b2 = __builtin_bit_cast(uint32_t, v2) + 0x10u, b3 = __builtin_bit_cast(uint32_t, v3) + 0x10u;
          typedef __fp16 pk2 __attribute__((ext_vector_type(2)));
          const pk2 h01 = __builtin_amdgcn_cvt_pkrtz(__builtin_bit_cast(float, b0), __builtin_bit_cast(float, b1));
          const pk2 h23 = __builtin_amdgcn_cvt_pkrtz(__builtin_bit_cast(float, b2), __builtin_bit_cast(float, b3));
          const uint32_t lo = ((b0 >> 5) & 0xffu) | (((b1 >> 5) & 0xffu) << 8) | (((b2 >> 5) & 0xffu) << 16) | ((b3 >> 5) << 24);
          u32x2 w8;
          w8[0] = s ? __builtin_bit_cast(uint32_t, h01) : __builtin_bit_cast(uint32_t, v0);
          w8[1] = s ? __builtin_bit_cast(uint32_t, h23) : __builtin_bit_cast(uint32_t, v1);
          *reinterpret_cast<u32x2*>(tl + 24 * q + 8 * hh) = w8;
          *reinterpret_cast<uint32_t*>(tl + 24 * q + 16 + 4 * hh) = s ? lo : __builtin_bit_cast(uint32_t, v2);
        }
      }
      if (!PARKD && j == 3 && more) park_m(buf ^ 1);
      DW_BAR();
    }
  }
  if (!(gh_max <= 65504.f)) *flag = 1;
}

template <typename F>
static float timeit(F f, int reps = 5) {
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  f();
  CK(hipDeviceSynchronize());
  float best = 1e9f;
  for (int i = 0; i < reps; ++i) {
    CK(hipEventRecord(e0));
    f();
    CK(hipEventRecord(e1));
    CK(hipEventSynchronize(e1));
    float ms;
    CK(hipEventElapsedTime(&ms, e0, e1));
    best = ms < best ? ms : best;
  }
  return best;
}

// D modes: rows per workgroup 256 / 512 / 1024, the x split on the store wave or on the MFMA waves
static void run_drainwave(float* out) {
  const size_t nx = (size_t)NROWS * DW_LDX, nw = (size_t)NZ * 2 * 4 * 2 * DW_NCOLS * 8;
  float* hx = (float*)malloc(nx * 4);
  _Float16* hw = (_Float16*)malloc(nw * 2);
  srand(1);
  for (size_t i = 0; i < nx; ++i) hx[i] = (float)(rand() % 2001 - 1000) * 1e-3f;
  for (size_t i = 0; i < nw; ++i) hw[i] = (_Float16)((float)(rand() % 2001 - 1000) * 1e-4f);
  float* x;
  _Float16* w;
  int* flag;
  CK(hipMalloc(&x, nx * 4));
  CK(hipMalloc(&w, nw * 2));
  CK(hipMalloc(&flag, 4));
  CK(hipMemcpy(x, hx, nx * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(w, hw, nw * 2, hipMemcpyHostToDevice));
  CK(hipMemset(flag, 0, 4));
  const double gb = (double)NZ * NROWS * DW_LD * 4 / 1e9;
  for (int mrows : {256, 512, 1024}) {
    const dim3 grid((DW_NG + 2) / 3, (NROWS + mrows - 1) / mrows, NZ);
    float ms = timeit([&] { hipLaunchKernelGGL((drainwave<true>), grid, dim3(256), 0, 0, x, w, out, NROWS, mrows, flag); }, 10);
    printf("D0 3 MFMA waves + 1 store wave (x split on the store wave), %4d rows per workgroup   %.3f ms  %.2f GB  %.2f TB/s\n", mrows, ms, gb, gb / ms);
    ms = timeit([&] { hipLaunchKernelGGL((drainwave<false>), grid, dim3(256), 0, 0, x, w, out, NROWS, mrows, flag); }, 10);
    printf("D1 3 MFMA waves + 1 store wave (x split on the MFMA waves),  %4d rows per workgroup   %.3f ms  %.2f GB  %.2f TB/s\n", mrows, ms, gb, gb / ms);
  }
  CK(hipGetLastError());
  int hf = 0;
  CK(hipMemcpy(&hf, flag, 4, hipMemcpyDeviceToHost));
  printf("(range flag %d)\n", hf);
  free(hx);
  free(hw);
}

int main(int argc, char** argv) {
  float* out;
  CK(hipMalloc(&out, (size_t)NZ * NROWS * LD0 * 4));
  if (argc > 1 && argv[1][0] == 'd') {   // `store_g3 dw`: the D modes only
    run_drainwave(out);
    return 0;
  }
  const dim3 grid((N8 * GCP + 63) / 64, (NROWS + 511) / 512, NZ);
  const double gb0 = (double)NZ * NROWS * N8 * GCP * 32 / 1e9, gb1 = (double)NZ * NROWS * N8 * GCP * 24 / 1e9;
  float ms;
  ms = timeit([&] { hipLaunchKernelGGL((drain<0>), grid, dim3(256), 0, 0, out, 512); });
  printf("F0 form 0: hi + lo 16-byte pieces interleaved (whole lines per store pair)   %.3f ms  %.2f GB  %.2f TB/s\n", ms, gb0, gb0 / ms);
  ms = timeit([&] { hipLaunchKernelGGL((drain<1>), grid, dim3(256), 0, 0, out, 512); });
  printf("G0 form 1: 16 rows x 64 B hi (x4) + 16 rows x 32 B lo (x2)                    %.3f ms  %.2f GB  %.2f TB/s\n", ms, gb1, gb1 / ms);
  ms = timeit([&] { hipLaunchKernelGGL((drain<2>), grid, dim3(256), 0, 0, out, 512); });
  printf("G1 form 1: lo as dwordx4 from every second lane                                %.3f ms  %.2f GB  %.2f TB/s\n", ms, gb1, gb1 / ms);
  ms = timeit([&] { hipLaunchKernelGGL((drain<3>), grid, dim3(256), 0, 0, out, 512); });
  printf("G2 form 1: a row tile's 8 hi stores back to back, then its 8 lo stores          %.3f ms  %.2f GB  %.2f TB/s\n", ms, gb1, gb1 / ms);
  ms = timeit([&] { hipLaunchKernelGGL((drain<4>), grid, dim3(256), 0, 0, out, 512); });
  printf("G3 hi region + lo region of 16-byte pieces (no byte saving)                    %.3f ms  %.2f GB  %.2f TB/s\n", ms, gb0, gb0 / ms);
  ms = timeit([&] { hipLaunchKernelGGL((drain<5>), grid, dim3(256), 0, 0, out, 512); });
  printf("G4 form 1 with non-temporal stores                                             %.3f ms  %.2f GB  %.2f TB/s\n", ms, gb1, gb1 / ms);
  ms = timeit([&] { hipLaunchKernelGGL((drain<6>), grid, dim3(256), 0, 0, out, 512); });
  printf("H0 24-byte units: dwordx4 + dwordx2 per block and half tile                    %.3f ms  %.2f GB  %.2f TB/s\n", ms, gb1, gb1 / ms);
  ms = timeit([&] { hipLaunchKernelGGL((drain<7>), grid, dim3(256), 0, 0, out, 512); });
  printf("H1 24-byte units as 12-byte pieces: one dwordx3 per lane, 8 rows x 96 B        %.3f ms  %.2f GB  %.2f TB/s\n", ms, gb1, gb1 / ms);
  ms = timeit([&] { hipLaunchKernelGGL((drain<8>), grid, dim3(256), 0, 0, out, 512); });
  printf("H2 ... the four blocks of a row group back to back                             %.3f ms  %.2f GB  %.2f TB/s\n", ms, gb1, gb1 / ms);
  // the same with the stores spaced as in the kernel: two workgroups per CU (70 KiB of dynamic LDS each), s_sleep(2) = ~128 cycles behind every store
  const size_t lds = 70 * 1024;
  CK(hipFuncSetAttribute(reinterpret_cast<const void*>(drain<0, 2>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  CK(hipFuncSetAttribute(reinterpret_cast<const void*>(drain<1, 2>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  CK(hipFuncSetAttribute(reinterpret_cast<const void*>(drain<6, 2>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  CK(hipFuncSetAttribute(reinterpret_cast<const void*>(drain<7, 2>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  CK(hipFuncSetAttribute(reinterpret_cast<const void*>(drain<8, 2>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  ms = timeit([&] { hipLaunchKernelGGL((drain<0, 2>), grid, dim3(256), lds, 0, out, 512); });
  printf("spaced, two workgroups per CU:  F0 %.3f ms %.2f TB/s", ms, gb0 / ms);
  ms = timeit([&] { hipLaunchKernelGGL((drain<1, 2>), grid, dim3(256), lds, 0, out, 512); });
  printf(" | G0 %.3f ms %.2f TB/s", ms, gb1 / ms);
  ms = timeit([&] { hipLaunchKernelGGL((drain<6, 2>), grid, dim3(256), lds, 0, out, 512); });
  printf(" | H0 %.3f ms %.2f TB/s", ms, gb1 / ms);
  ms = timeit([&] { hipLaunchKernelGGL((drain<7, 2>), grid, dim3(256), lds, 0, out, 512); });
  printf(" | H1 %.3f ms %.2f TB/s", ms, gb1 / ms);
  ms = timeit([&] { hipLaunchKernelGGL((drain<8, 2>), grid, dim3(256), lds, 0, out, 512); });
  printf(" | H2 %.3f ms %.2f TB/s\n", ms, gb1 / ms);
  run_drainwave(out);
  return 0;
}
