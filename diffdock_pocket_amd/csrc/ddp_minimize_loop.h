// ddp_minimize_loop.h - the line search of the fused minimiser as a device function: the LDS plan, the evaluation of E, the pose map on
// the plan's carve and the iteration loop with its single call site of the evaluation.  ddp_pose_minimize_kernel (ddp_minimize.hip)
// runs it once per pose, ddp_pose_search_kernel (ddp_search.hip) once per cycle of a replica.  Both are one 256-thread workgroup per
// row; diffdock_pocket_amd/minimize.py states the algorithm.  The functions are templated on the argument struct, as score_evaluate
// of ddp_pose_descent.h is: what they read of it is n, m, n_tor, bonds, mask_rotate, rec_radii, rec_flags, self_pairs, form, restraint,
// grow, shrink and step_max.  The energy of a pose is a function of its fp32 coordinates and the anchor only, whichever kernel,
// iteration or launch evaluates it: that is what makes the kernels resumable and comparable bit for bit.
#ifndef DDP_MINIMIZE_LOOP_H
#define DDP_MINIMIZE_LOOP_H
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ddp_hip.h"
#include "ddp_internal.h"
#include "ddp_horn.h"
#include "ddp_pose_descent.h"

#define DDP_MZ_THREADS DDP_DESCENT_THREADS
#define DDP_MZ_WAVES DDP_DESCENT_WAVES
#define DDP_MZ_TILE DDP_SCORE_TILE
// fixed part of the LDS plan, every carve a multiple of 16 bytes: the receptor tile and its flag bytes, then the reduction scratch
#define DDP_MZ_WE_BYTES (DDP_MZ_WAVES * 10 * 8)      // [waves][8] fp64: the energy partials of score_evaluate, then [waves] of the restraint
#define DDP_MZ_RED_BYTES (DDP_MZ_WAVES * 16 * 8)     // fp64 or fp32: block sums of the direction and the pose map (at most [waves][9])
#define DDP_MZ_FIXED_BYTES (DDP_MZ_TILE * 16 + DDP_MZ_TILE + DDP_MZ_WE_BYTES + DDP_MZ_RED_BYTES + 64)

static_assert(DDP_MINIMIZE_MAX_TORSIONS * sizeof(float) <= DDP_MZ_TILE * sizeof(float4), "the torsion steps live in the tile between two evaluations");
static_assert(DDP_MZ_FIXED_BYTES % 16 == 0, "dynamic LDS carves stay 16-byte aligned");
static_assert(DDP_MZ_FIXED_BYTES + 89 * DDP_MINIMIZE_MAX_ATOMS <= 64 * 1024, "the LDS plan fits the 64 KiB a plain launch may ask for");

struct MzLds {
  float4* tile;        // [DDP_MZ_TILE] receptor x, y, z, radius; between two evaluations its first floats hold the torsion steps
  uint8_t* tflag;      // [DDP_MZ_TILE]
  double (*we)[8];     // [waves][8]
  double* wr;          // [waves] the restraint sums of the waves
  double* red;         // scratch of block_sum
  double* et;          // [4] the energies of the last evaluation
  double* g;           // [2][n][3] gradients: of the current pose and of the trial (which is which changes with every accept)
  float* x;            // [2][n][3] the current pose and the trial
  float* rg;           // [n][3] the rigid copy of the pose map
  float* rad;          // [n]
  uint8_t* lflag;      // [n]
};

// the plan on a dynamic LDS block of mz_lds_bytes(n) bytes: the fixed part (receptor tile, its flags, reduction scratch) + two
// gradients, three coordinate sets, radii and flags per atom: 17.9 KiB + 89 n, 62.4 KiB at the atom limit
static inline size_t mz_lds_bytes(int n) { return DDP_MZ_FIXED_BYTES + (size_t)89 * n; }

__device__ __forceinline__ MzLds mz_carve(unsigned char* p, int n) {
  MzLds L;
  L.tile = (float4*)p; p += DDP_MZ_TILE * sizeof(float4);
  L.tflag = p; p += DDP_MZ_TILE;
  L.we = (double(*)[8])p; L.wr = (double*)p + DDP_MZ_WAVES * 8; p += DDP_MZ_WE_BYTES;
  L.red = (double*)p; p += DDP_MZ_RED_BYTES;
  L.et = (double*)p; p += 64;
  L.g = (double*)p; p += (size_t)48 * n;
  L.x = (float*)p; p += (size_t)24 * n;
  L.rg = (float*)p; p += (size_t)12 * n;
  L.rad = (float*)p; p += (size_t)4 * n;
  L.lflag = p;
  return L;
}

// Energy [inter, intra, restraint term, E] -> L.et and gradient -> g of the pose x (LDS, visible to all threads on entry).  Ends with
// a barrier: L.et and g are visible on return.  score_evaluate, then the restraint of ddp_refine_energy_kernel in a pass of its own:
// wave w sums its atoms w, w + 4, ... in that order (all lanes hold the same value), the waves are added in wave order.
template <class Args>
__device__ __forceinline__ void mz_evaluate(const Args& A, const MzLds& L, const float* __restrict__ rs, const float* __restrict__ as,
                                            const float* x, double* g) {
  const int tid = threadIdx.x, n = A.n;
  score_evaluate<true>(A, rs, L.tile, L.tflag, x, L.rad, L.lflag, g, L.we);
  descent_ligand_restraint(A, x, as, g, L.wr);
  __syncthreads();
  if (tid == 0) {
    double t[8], inter, intra, er = L.wr[0];
    score_totals(A.form, L.we, t, inter, intra);
    for (int w = 1; w < DDP_MZ_WAVES; ++w) er += L.wr[w];
    const double rest = A.restraint * (er / (double)n);
    L.et[0] = inter; L.et[1] = intra; L.et[2] = rest; L.et[3] = (inter + intra) + rest;
  }
  __syncthreads();
}

// xt = the pose map of ddp_pose_update_kernel applied to x with (tr, rot, tor): descent_pose_update of ddp_pose_descent.h on this plan's
// carve (the torsion steps in the tile's first floats, visible on entry).  Ends with a barrier: xt is visible on return.
template <class Args>
__device__ __forceinline__ void mz_pose_update(const Args& A, const MzLds& L, const float* x, float* xt, const float* tr, const float* rot) {
  descent_pose_update(A, x, xt, L.rg, (const float*)L.tile, (float*)L.red, tr, rot);
}

// `iterations` iterations of the line search.  On entry the start pose lies in the TRIAL buffer L.x + (cur ^ 1) 3 n and the radii and
// flags in L.rad / L.lflag, all visible (a barrier behind them); pass 0 of the loop evaluates the start pose and takes it whatever its
// energy.  On return the pose lies in L.x + cur 3 n and its gradient in L.g + cur 3 n (cur has flipped once per pose taken), e[4] holds
// its energies and e0[4] those of the start pose, step and taken have been advanced; every thread holds the same values, read from
// the same LDS words.  hist (or NULL): thread 0 writes E before the first and after every iteration to hist[it hist_stride].
// rs: the row's receptor, as: its anchor (global memory).  There is exactly ONE call site of the evaluation.  No data-dependent
// control flow around a barrier: the trip count is an argument, the accept decision follows the last barrier of the evaluation.
template <class Args>
__device__ __forceinline__ void mz_descend(const Args& A, const MzLds& L, const float* __restrict__ rs, const float* __restrict__ as,
                                           int iterations, int& cur, double& step, int& taken, double* e, double* e0, double* hist,
                                           size_t hist_stride) {
  const int tid = threadIdx.x, n = A.n;
  for (int it = 0; it <= iterations; ++it) {
    if (it > 0) {
      // the torsion steps go to the tile's first n_tor floats; the barrier makes them visible
      float tr[3], rot[3];
      descent_direction<true>(L.x + cur * 3 * n, L.g + cur * 3 * n, n, A.n_tor, A.bonds, A.mask_rotate, step, L.red, tr, rot, (float*)L.tile);
      __syncthreads();
      mz_pose_update(A, L, L.x + cur * 3 * n, L.x + (cur ^ 1) * 3 * n, tr, rot);
    }
    mz_evaluate(A, L, rs, as, L.x + (cur ^ 1) * 3 * n, L.g + (cur ^ 1) * 3 * n);
    const double et3 = L.et[3];
    const bool take = it == 0 || et3 < e[3];     // strict, fp64, false for NaN; the same LDS words for every thread
    if (take) {
      e[0] = L.et[0]; e[1] = L.et[1]; e[2] = L.et[2]; e[3] = et3;
      cur ^= 1;
    }
    if (it > 0) {
      step = take ? fmin(A.grow * step, A.step_max) : A.shrink * step;
      taken += take ? 1 : 0;
    } else {
      e0[0] = e[0]; e0[1] = e[1]; e0[2] = e[2]; e0[3] = e[3];
    }
    if (hist && tid == 0) hist[(size_t)it * hist_stride] = e[3];
    // (the next write of L.et lies behind the barriers of the next evaluation)
  }
}

#endif
