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

#include "ddp_minimize_loop.h"

// The LDS plan, the evaluation, the pose map and the loop are ddp_minimize_loop.h's (the search of ddp_search.hip runs the same loop
// once per cycle); this kernel stages a pose, runs the loop once and writes the state back.
__global__ __launch_bounds__(DDP_MZ_THREADS) void ddp_pose_minimize_kernel(const ddp_minimize_args_t A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char mz_lds[];
  const int s = blockIdx.x, tid = threadIdx.x, n = A.n, S = A.n_samples;
  const MzLds L = mz_carve(mz_lds, n);
  float* gpos = A.pos + (size_t)s * n * 3;
  const float* __restrict__ as = A.anchor + (size_t)s * n * 3;
  const float* __restrict__ rs = A.rec + (size_t)s * A.rec_stride;
  // the start pose goes into the TRIAL buffer: pass 0 of the loop evaluates it and takes it whatever its energy
  int cur = 0;
  for (int i = tid; i < 3 * n; i += DDP_MZ_THREADS) L.x[3 * n + i] = gpos[i];
  for (int i = tid; i < n; i += DDP_MZ_THREADS) { L.rad[i] = A.lig_radii[i]; L.lflag[i] = A.lig_flags[i]; }
  double step = A.step[s];
  int taken = 0;
  double e[4] = {0.0, 0.0, 0.0, 0.0}, e0[4] = {0.0, 0.0, 0.0, 0.0};
  __syncthreads();
  mz_descend(A, L, rs, as, A.iterations, cur, step, taken, e, e0, A.history ? A.history + s : nullptr, (size_t)S);
  if (tid == 0) {
    double* ei = A.energy_in + 4 * (size_t)s;
    double* eo = A.energy_out + 4 * (size_t)s;
    ei[0] = e0[0]; ei[1] = e0[1]; ei[2] = e0[2]; ei[3] = e0[3];
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
  const size_t lds = mz_lds_bytes(a->n);     // 17.9 KiB + 89 n, 62.4 KiB at the atom limit
  hipLaunchKernelGGL(ddp_pose_minimize_kernel, dim3(a->n_samples), dim3(DDP_MZ_THREADS), lds, (hipStream_t)stream, *a);
  return ddp_launch_result("ddp_pose_minimize");
}
