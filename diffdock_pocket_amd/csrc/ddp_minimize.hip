// ddp_minimize.hip - local minimisation of sampled poses in the Vinardo-form score, the whole backtracking line search of a pose in
// ONE launch (include/ddp_hip.h, ddp_pose_minimize; host side diffdock_pocket_amd/minimize.py, which states the whole definition).
// The launch-by-launch form of the same loop (ddp_pose_score, ddp_refine_direction, ddp_pose_update, ddp_refine_accept) pays four to
// five dependent launches per iteration, and the launches, not the arithmetic, are its cost.  Every pose is independent and one
// workgroup already holds a whole pose, so here one 256-thread workgroup runs all iterations of its pose: the current pose, the trial,
// the rigid copy of the pose map, both gradients, the radii and the flags stay in LDS for the whole call.
// Per iteration: descent_direction of ddp_pose_descent.h (the one definition, ddp_refine_direction_kernel calls it too); the pose map
// of ddp_pose_update_kernel in fp32 (rigid move about the centroid, the torsions in bond order, Horn re-alignment through ddp_horn.h:
// every thread runs the 4x4 Jacobi on the same block sums, which costs a SIMD what one thread costs it and saves the barrier that
// publishing the matrix would need; only the block sums are this kernel's own, see mz_pose_update); energy and gradient of the trial
// through score_evaluate of ddp_pose_descent.h (the one definition, ddp_pose_score_kernel calls it too) plus the restraint; the accept
// decision, which every thread takes from the same LDS words after a barrier: it is workgroup-uniform.
// There is exactly ONE call site of the evaluation (the start pose goes through it as a trial that is always taken), so the energy of
// a pose is a function of its fp32 coordinates and the anchor only, whichever iteration or launch evaluates it: a call with a + b
// iterations equals a call with a and a call with b.  No atomics, every sum in a fixed order, no receptor pruning.
// No data-dependent control flow around a barrier: the trip counts are kernel arguments, the conditions that skip a barrier (a bonds
// entry outside the ligand, n_tor = 0) are the same for all 256 threads, the Jacobi sweep has its fixed bound of 30.
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

// Energy [inter, intra, restraint term, E] -> L.et and gradient -> g of the pose x (LDS, visible to all threads on entry).  Ends with
// a barrier: L.et and g are visible on return.  score_evaluate, then the restraint of ddp_refine_energy_kernel in a pass of its own:
// wave w sums its atoms w, w + 4, ... in that order (all lanes hold the same value), the waves are added in wave order.
__device__ __forceinline__ void mz_evaluate(const ddp_minimize_args_t& A, const MzLds& L, const float* __restrict__ rs,
                                         const float* __restrict__ as, const float* x, double* g) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = A.n;
  score_evaluate<true>(A, rs, L.tile, L.tflag, x, L.rad, L.lflag, g, L.we);
  const double krest = 2.0 * A.restraint / (double)n;
  double er_w = 0.0;
  for (int i = wave; i < n; i += DDP_MZ_WAVES) {
    const double xi = x[3 * i], yi = x[3 * i + 1], zi = x[3 * i + 2];
    const double ax = xi - (double)as[3 * i], ay = yi - (double)as[3 * i + 1], az = zi - (double)as[3 * i + 2];
    er_w += ax * ax + ay * ay + az * az;
    if (lane == 0) { g[3 * i] = g[3 * i] + krest * ax; g[3 * i + 1] = g[3 * i + 1] + krest * ay; g[3 * i + 2] = g[3 * i + 2] + krest * az; }
  }
  if (lane == 0) L.wr[wave] = er_w;
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

// xt = the pose map of ddp_pose_update_kernel applied to x with (tr, rot, tor): descent_pose_update of ddp_pose_descent.h on this kernel's
// carve (the torsion steps in the tile's first floats).  Ends with a barrier: xt is visible on return.
__device__ __forceinline__ void mz_pose_update(const ddp_minimize_args_t& A, const MzLds& L, const float* x, float* xt, const float* tr,
                                               const float* rot) {
  descent_pose_update(A, x, xt, L.rg, (const float*)L.tile, (float*)L.red, tr, rot);
}

__global__ __launch_bounds__(DDP_MZ_THREADS) void ddp_pose_minimize_kernel(const ddp_minimize_args_t A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char mz_lds[];
  const int s = blockIdx.x, tid = threadIdx.x, n = A.n, S = A.n_samples;
  MzLds L;
  unsigned char* p = mz_lds;
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
  float* gpos = A.pos + (size_t)s * n * 3;
  const float* __restrict__ as = A.anchor + (size_t)s * n * 3;
  const float* __restrict__ rs = A.rec + (size_t)s * A.rec_stride;
  // the start pose goes into the TRIAL buffer: pass 0 of the loop evaluates it and takes it whatever its energy
  int cur = 0;
  for (int i = tid; i < 3 * n; i += DDP_MZ_THREADS) L.x[3 * n + i] = gpos[i];
  for (int i = tid; i < n; i += DDP_MZ_THREADS) { L.rad[i] = A.lig_radii[i]; L.lflag[i] = A.lig_flags[i]; }
  double step = A.step[s];
  int taken = 0;
  double e[4] = {0.0, 0.0, 0.0, 0.0};
  __syncthreads();
  for (int it = 0; it <= A.iterations; ++it) {
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
    } else if (tid == 0) {
      double* ei = A.energy_in + 4 * (size_t)s;
      ei[0] = e[0]; ei[1] = e[1]; ei[2] = e[2]; ei[3] = e[3];
    }
    if (A.history && tid == 0) A.history[(size_t)it * S + s] = e[3];
    // (the next write of L.et lies behind the barriers of the next evaluation)
  }
  if (tid == 0) {
    double* eo = A.energy_out + 4 * (size_t)s;
    eo[0] = e[0]; eo[1] = e[1]; eo[2] = e[2]; eo[3] = e[3];
  }
  if (A.iterations > 0 && tid == 0) { A.step[s] = step; A.accepted[s] += taken; }
  if (taken > 0)
    for (int i = tid; i < 3 * n; i += DDP_MZ_THREADS) gpos[i] = L.x[cur * 3 * n + i];
  if (A.grad) {
    double* go = A.grad + (size_t)s * n * 3;
    for (int i = tid; i < 3 * n; i += DDP_MZ_THREADS) go[i] = L.g[cur * 3 * n + i];
  }
}

extern "C" int ddp_pose_minimize(const ddp_minimize_args_t* a, void* stream) {
  if (!a) return ddp_fail(DDP_EINVAL, "ddp_pose_minimize: null argument struct");
  if (a->n_samples == 0) return 0;
  if (const int rc = ddp_pose_check_shape("ddp_pose_minimize", a->n_samples, a->n, a->m, a->rec_stride, a->n_tor >= 0)) return rc;
  if (const int rc = DDP_POSE_CHECK_ATOMS("ddp_pose_minimize", a->n, DDP_MINIMIZE_MAX_ATOMS)) return rc;
  if (a->n_tor > DDP_MINIMIZE_MAX_TORSIONS) return ddp_fail(DDP_ELIMIT, "ddp_pose_minimize: more than DDP_MINIMIZE_MAX_TORSIONS rotatable bonds");
  if (!a->pos || !a->anchor || !a->lig_radii || !a->lig_flags || !a->step || !a->accepted || !a->energy_in || !a->energy_out ||
      (a->m > 0 && (!a->rec || !a->rec_radii || !a->rec_flags)) || (a->n_tor > 0 && (!a->bonds || !a->mask_rotate)))
    return ddp_fail(DDP_EINVAL, "ddp_pose_minimize: null argument");
  if (a->iterations < 0 || !(a->restraint >= 0.0)) return ddp_fail(DDP_EINVAL, "ddp_pose_minimize: iterations or restraint < 0");
  if (const int rc = score_check_constants(&a->form, "ddp_pose_minimize")) return rc;
  // the fixed part (receptor tile, its flags, reduction scratch) + two gradients, three coordinate sets, radii and flags per atom:
  // 17.9 KiB + 89 n, 62.4 KiB at the atom limit
  const size_t lds = DDP_MZ_FIXED_BYTES + (size_t)89 * a->n;
  hipLaunchKernelGGL(ddp_pose_minimize_kernel, dim3(a->n_samples), dim3(DDP_MZ_THREADS), lds, (hipStream_t)stream, *a);
  return ddp_launch_result("ddp_pose_minimize");
}
