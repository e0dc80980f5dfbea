// ddp_conv_rows_common.h - what the two forms of the row-stationary conv kernel share: ddp_conv_rows.hip (form 0, v_mfma_f32_32x32x16_f16)
// and ddp_conv_rows16.hip (form 1, v_mfma_f32_16x16x32_f16; ddp_conv_task_t::rows_form).  Everything here is independent of the MFMA
// shape: the workgroup constants and plane scales, the per-edge tables of a wave, the weight stream through the three-slot LDS ring, the
// basis features of the vector-input segments, the byte layout of G inside a node's row, and - on the host - the one launch plan.  Every
// device function is __forceinline__: both units compile to the instructions they had with private copies
// (profiles/rows_common_isa.txt).
#ifndef DDP_CONV_ROWS_COMMON_H
#define DDP_CONV_ROWS_COMMON_H
#include "ddp_conv_common.h"

#define ROWS_NW 4      // waves per workgroup
#define ROWS_NT 256
#define ROWS_ET 128    // edges per workgroup: 32 per wave
#define ROWS_FS 36     // floats per feature row F[u * C + c][edge]
#define ROWS_NP 3      // pieces per stream tile (one ring slot each)
#define R16_FROWS 72   // form 1: feature rows a wave holds at a time (a block with more - the direct convs: 80 features x 3 components - builds them in chunks)

// Operand planes of the kernel ("unified" fp16 hi/lo planes, include/ddp_hip.h DDP_ROWS_S*): V = v * 2^s = hi + lo with hi = fp16(V),
// lo = fp16(V - hi) at the SAME scale, so that the three split products hh wh + hh wl + hl wh land in ONE accumulator (the common form
// v = hi + lo / 2048 of ddp_conv_common.h needs two and a multiply-add per element to join them: 32 registers of every tile product
// here).  22 significant bits while lo is a normal fp16 number (|V| >= 0.125), an absolute 2^-25 / 2^s below; |V| <= 65504 or the
// range flag is raised.  The accumulators carry 2^(sa + sb); the feature rows / harmonics they are multiplied with carry the inverse.
#define ROWS_SX ((float)DDP_ROWS_SX)
#define ROWS_SW ((float)DDP_ROWS_SW)
#define ROWS_SH ((float)DDP_ROWS_SH)
#define ROWS_SG ((float)DDP_ROWS_SG)
__device__ __forceinline__ void rows_split(const f32x4 v, float scale, h4& hi, h4& lo, int32_t* flag) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float V = v[i] * scale;
    h2_range_check(V, flag);
    hi[i] = (_Float16)V;
    lo[i] = (_Float16)(V - (float)hi[i]);
  }
}

// The kernel arguments of the two forms (field order and size are part of every kernel's instructions)
struct RowsLaunch {
  ConvLaunch L;
  int nts;         // stream tiles per conv (fc.0 tiles + fc.3 tiles of all segments)
  int bias_bytes;  // LDS bytes of the bias table behind the ring
  int priv_bytes;  // LDS bytes of a wave's private area
  int aux_off;     // byte offset of the per-edge tables inside it
};
struct R16Launch {
  ConvLaunch L;
  int nts;         // stream tiles per conv (fc.0 tiles + fc.3 tiles of all segments)
  int bias_tiles;  // stream tiles whose bias words sit in the LDS table (all, or fc.0's: ddp_conv_task_t::rows_bias_k)
  int bias_bytes;  // LDS bytes of the bias table behind the ring
  int priv_bytes;  // LDS bytes of a wave's private area
  int aux_off;     // byte offset of the per-edge tables inside it
  int frows;       // feature rows of the private area (<= R16_FROWS)
};
static_assert(sizeof(ConvLaunch) + 16 <= 4096, "the launch descriptor travels as a kernel argument");

// per-edge tables of a wave (behind its feature rows)
struct RowsAux {
  float shT[4][32];   // harmonics, component-major (the "feature rows" of the factorised features), x 1 / (SH SG)
  float sh[32][4];    // ... edge-major, x 1 / (SH SW) (the stream tiles' features; build_features)
  int src[32], pos[32], rid[32];
};

// The weight stream: a tile travels as ROWS_NP pieces of NS / ROWS_NP k-steps (8 KiB at NS = 12), piece p of every tile through slot p of
// a three-slot LDS ring.  One stream step j = ROWS_NP t + p: every wave's part of piece j has landed (the wave waits for its own LDS-DMA
// copies of piece j - those of piece j + 1 stay in flight - then the barrier), nobody reads piece j - 1 any more, so piece j + 2 is
// requested into its slot (no staging registers; every wave moves 2 NS / (ROWS_NP ROWS_NW) fragments of 1 KiB, lane-linear in LDS).  A
// copy has two piece products to land (one was not enough: ~1 k ticks of every 3.4 k-tick tile waited for it).
typedef __attribute__((address_space(3))) void* rows_lds_ptr_t;
// (the copies are BUFFER loads to LDS, not global_load_lds: hipcc books a global_load_lds as a flat access to both address spaces, and while
// one is pending every wait for an ordinary load becomes vmcnt(0))
typedef __amdgpu_buffer_rsrc_t RowsStream;
__device__ __forceinline__ RowsStream rows_stream_of(const void* wsh, int nts, int tile_bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(wsh), 0, nts * tile_bytes, 0x00020000);
}
template <int NS>
__device__ __forceinline__ void rows_request_piece(f32x4* ring, RowsStream wsh, int jn, int npieces, int slot, int wave, int lane) {
  constexpr int FPP = 2 * NS / ROWS_NP, FPW = FPP / ROWS_NW, PIECE_Q = FPP * 64;
  static_assert(NS % ROWS_NP == 0 && FPP % ROWS_NW == 0, "every wave moves the same number of fragments per piece");
  f32x4* nslot = ring + slot * PIECE_Q;
  const int piece_off = min(jn, npieces - 1) * (PIECE_Q * 16);
#pragma unroll
  for (int f = 0; f < FPW; ++f)
    __builtin_amdgcn_raw_ptr_buffer_load_lds(wsh, (rows_lds_ptr_t)(nslot + (wave + ROWS_NW * f) * 64), 16, ((wave + ROWS_NW * f) * 64 + lane) * 16, piece_off, 0, 0);
}
template <int NS, int P>
__device__ __forceinline__ void rows_stream_step(f32x4* ring, RowsStream wsh, int t, int nts, int wave, int lane) {
  constexpr int FPW = 2 * NS / ROWS_NP / ROWS_NW;
  // (hipcc does NOT wait for an LDS-DMA in front of a barrier: without this a wave can pass while its part of the piece is in flight.
  // vmcnt counts in order: "at most FPW outstanding" = everything older than the copies of piece j + 1 has landed)
  static_assert(FPW == 2 || FPW == 1, "the literals below");
  if constexpr (FPW == 2)
    asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
  else
    asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
  // the bare barrier, not __syncthreads(): its workgroup fence makes hipcc wait vmcnt(0) whenever an ordinary load is in flight.  What
  // the barrier orders here is LDS only: this wave's reads of the slot that is requested next (and, once, the bias table's writes) are
  // complete (lgkmcnt(0)), the copies it waits for are counted above; the asm statements keep the compiler from moving LDS accesses
  // across it.
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  rows_request_piece<NS>(ring, wsh, ROWS_NP * t + P + 2, ROWS_NP * nts, (P + 2) % ROWS_NP, wave, lane);
}

// The basis features of a block's vector-input segments (DOT, VEC_S0, CROSS; build_features of ddp_conv_common.h restated for one wave;
// independent of the MFMA shape - feature rows are indexed by edge): ALL loads of a segment first - clamped, unconditional - then the
// arithmetic.  build_features issues one load per feature inside a runtime loop, and with the stream's LDS-DMA copies in flight hipcc
// waits vmcnt(0) at every use: ~700 ticks per feature, 6 - 13 k per block.
template <int MAXI>
__device__ __forceinline__ void rows_build_features(const ddp_block_t& B, const ddp_conv_task_t& T, const RowsAux* aux, float* F, int lane) {
  constexpr int FS = ROWS_FS;
  const int e = lane & 31, half = lane >> 5;
  const float* __restrict__ xrow = T.x_src + (size_t)aux->src[e] * T.ldx_src;
  // (aux->sh carries 1 / (DDP_ROWS_SH DDP_ROWS_SW): the stream tiles' accumulators carry the planes' scales)
  const float s0 = aux->sh[e][0], sx = aux->sh[e][1], sy = aux->sh[e][2], sz = aux->sh[e][3];
  const float inv_sqrt3 = 0.57735026918962576f, inv_sqrt2 = 0.70710678118654752f;
  int ubase = 0;
  for (int si = 0; si < B.nseg; ++si) {
    const int kind = B.seg[si].kind, off = B.seg[si].in_off, cnt = B.seg[si].count;
    float ax[MAXI], ay[MAXI], az[MAXI];
#pragma unroll
    for (int i = 0; i < MAXI; ++i) {
      const int ul = max(min(half + 2 * i, cnt - 1), 0);      // (an empty segment: the load stays inside the row, nothing is stored)
      ax[i] = xrow[off + 3 * ul];
      ay[i] = xrow[off + 3 * ul + 1];
      az[i] = xrow[off + 3 * ul + 2];
    }
#pragma unroll
    for (int i = 0; i < MAXI; ++i) {
      const int ul = half + 2 * i;
      if (ul < cnt) {
        const int u = ubase + ul;
        if (kind == DDP_F_DOT) {
          F[u * FS + e] = (ax[i] * sx + ay[i] * sy + az[i] * sz) * inv_sqrt3;
        } else if (kind == DDP_F_VEC_S0) {
          F[(u * 3 + 0) * FS + e] = ax[i] * s0;
          F[(u * 3 + 1) * FS + e] = ay[i] * s0;
          F[(u * 3 + 2) * FS + e] = az[i] * s0;
        } else {  // DDP_F_CROSS: a x s1 / sqrt(2)
          F[(u * 3 + 0) * FS + e] = (ay[i] * sz - az[i] * sy) * inv_sqrt2;
          F[(u * 3 + 1) * FS + e] = (az[i] * sx - ax[i] * sz) * inv_sqrt2;
          F[(u * 3 + 2) * FS + e] = (ax[i] * sy - ay[i] * sx) * inv_sqrt2;
        }
      }
    }
    ubase += cnt;
  }
}

// Where the G tile of segment (block bi, part) sits inside a node's row of task.gh[slot] (include/ddp_hip.h, ddp_conv_task_t::gh).  G of
// a source node and slot: the column parts of the slot's blocks one after the other, each a CONTIGUOUS tile [k8][wp columns][plane]
// [8 halves] (wp = the part's width rounded up to 4), then Gb per padded column - a run reads one tile as one linear stream, and stage A
// fills it in whole 128-byte lines.
struct RowsGPart {
  const char* base;      // the part's tile inside node 0's row of its G array
  size_t gldb;           // node stride in bytes
  int wp, nmine, bias_off;   // padded width, columns, byte offset of Gb[column 0] (plane form 1: of the Gb region) from `base`
  int cumw;              // padded columns of the slot in front of the part
};
// Plane form GF of a G array (ddp_conv_task_t::gh_fmt): 0 = 32 bytes per unit (k8, c) as above; 1 (round 6: "G3"; ABI 17) = 24 bytes -
// 8 fp16 hi words (V truncated), then 8 continuation bytes (19 significant bits; include/ddp_hip.h); Gb per padded column c of the slot
// sits behind the units of all parts in 24-byte groups of six fp32: 24 (c / 6) + 4 (c % 6) bytes.
// ROWS_GPART_FILL: RowsGPart P_ of part `part_` of block B_ from the walk's results - the part's padded width wp_, the padded columns
// cumw_ of its slot in front of it and gcp_ of the whole slot.  A macro, not a function: the walk exists in two spellings (below and in
// ddp_conv_rows.hip), and each unit keeps its kernels' instructions only if the walk and this arithmetic are simplified as ONE function.
#define ROWS_GPART_FILL(GF_, P_, S_, T_, B_, part_, wp_, cumw_, gcp_)                                            \
  {                                                                                                              \
    const int n8 = ((S_).hid + 7) >> 3;                                                                          \
    if constexpr ((GF_) == 1) {                                                                                  \
      (P_).base = reinterpret_cast<const char*>((T_).gh[(B_).g_slot]) + (size_t)(n8 * (cumw_)) * 24;             \
      (P_).gldb = (size_t)DDP_GH3_LD((S_).hid, (gcp_)) * 4;                                                      \
      (P_).bias_off = n8 * ((gcp_) - (cumw_)) * 24;                                                              \
    } else {                                                                                                     \
      (P_).base = reinterpret_cast<const char*>((T_).gh[(B_).g_slot]) + (size_t)(2 * n8 * (cumw_)) * 16;         \
      (P_).gldb = (size_t)DDP_GH_LD((S_).hid, (gcp_)) * 4;                                                       \
      (P_).bias_off = (8 * n8 * (gcp_) + (cumw_)) * 4 - (2 * n8 * (cumw_)) * 16;                                 \
    }                                                                                                            \
    (P_).wp = (wp_);                                                                                             \
    (P_).nmine = min(32, (B_).n - 32 * (part_));                                                                 \
    (P_).cumw = (cumw_);                                                                                         \
  }
// The walk over the parts of the slot's blocks (the block must have a G part)
template <int GF>
__device__ __forceinline__ RowsGPart rows_gpart_of(const ddp_conv_shape_t& S, const ddp_conv_task_t& T, int bi, int part) {
  const ddp_block_t& B = S.blk[bi];
  int wp = 0, cumw = 0, gcp = 0;
  for (int bj = 0; bj < S.nblocks; ++bj) {
    const ddp_block_t& Bj = S.blk[bj];
    if (Bj.g_slot != B.g_slot) continue;
    for (int pj = 0; pj < ((Bj.n + 31) >> 5); ++pj) {
      const int wj = (min(32, Bj.n - 32 * pj) + 3) & ~3;
      if (bj < bi || (bj == bi && pj < part)) cumw += wj;
      if (bj == bi && pj == part) wp = wj;
      gcp += wj;
    }
  }
  RowsGPart P;
  ROWS_GPART_FILL(GF, P, S, T, B, part, wp, cumw, gcp)
  return P;
}

// ------------------------------------------------------------------------------------------------ host
// Everything of a ddp_conv_rows call up to the launch, for both forms (ddp_conv_rows_plan, csrc/ddp_conv_rows.hip): the checked
// arguments, the tasks with edges and their tile table, and the LDS plan.  The launchers copy from it into their kernel arguments.
struct RowsPlan {
  ConvLaunch L;       // shape, the tasks with edges, tile_start, dev_counts
  int sc;             // size class: 60 or 32
  int form, gh_fmt;   // rows_form and gh_fmt of the launch's tasks
  int tiles;          // workgroups (0: every task is empty, nothing to launch)
  int nts;            // stream tiles per conv
  int bias_tiles;     // ... whose bias words sit in the LDS table
  int bias_bytes, priv_bytes, aux_off;
  int frows;          // feature rows of a wave's private area
  size_t lds_bytes;   // dynamic LDS of the launch
};
int ddp_conv_rows_plan(const ddp_conv_shape_t* shape, const ddp_conv_task_t* tasks, int ntasks, RowsPlan* plan);
// csrc/ddp_conv_rows16.hip: the launch of ddp_conv_rows for a plan of form 1
int ddp_conv_rows16_launch(const RowsPlan& P, void* stream);

// one instantiation: raise its dynamic-LDS limit if this launch needs more (lds_have[]: one slot per instantiation), then launch.  Expects
// P (the plan), RL (the kernel argument), stream, err and lds_have[] in scope.
#define ROWS_LAUNCH(KERNEL_, SLOT_, WHERE_)                                                                          \
  {                                                                                                                  \
    err = ddp_need_lds(reinterpret_cast<const void*>(KERNEL_), (int)P.lds_bytes, &lds_have[SLOT_]);                  \
    if (err != hipSuccess) return ddp_fail_hip(err, WHERE_);                                                         \
    hipLaunchKernelGGL(KERNEL_, dim3(P.tiles), dim3(ROWS_NT), P.lds_bytes, (hipStream_t)stream, RL);                 \
  }

#endif
