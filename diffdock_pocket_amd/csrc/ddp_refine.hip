// ddp_refine.hip - steric-clash relief of sampled poses in pose space (include/ddp_hip.h, ddp_refine_energy / ddp_refine_direction /
// ddp_refine_accept; host side diffdock_pocket_amd/refine.py).  This project's own algorithm, not the reference's --relax (an OpenMM
// minimisation): a clash penalty on the clash rule of ddp_pose_contacts plus a restraint to the sampled pose, descended along the
// sampler's own degrees of freedom (translation, rotation, torsions) through ddp_pose_update, with a per-sample backtracking line
// search whose state (energies, step sizes, accept counters) lives in device memory.
// ddp_pose_update re-aligns the conformer after the torsions, so the torsion component of the search direction is NOT the exact
// derivative of the map that is applied: the direction is a heuristic, the strict accept rule of ddp_refine_accept (E(trial) < E(x)
// in fp64) is what guarantees descent.
// One 256-thread workgroup per sample.  All arithmetic is fp64 on the fp32 inputs (converted first).  Every sum has a fixed order,
// through the reductions of ddp_pose_descent.h, which also holds the search direction (shared with the fused minimiser).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "ddp_hip.h"
#include "ddp_internal.h"
#include "ddp_clash_energy.h"
#include "ddp_pose_descent.h"

// ---- energy[s] = [E_cross, E_self, E_rest, total], grad[s][i] = dE/dx_i: the pass of ddp_clash_energy.h (shared with the guidance term
// of ddp_guidance.hip).  LDS: the sample's ligand coordinates and radii (fp32), one fp64 gradient accumulator per ligand atom, and a
// tile of DDP_REFINE_TILE receptor atoms.  Per-wave energy partials are summed over the waves in wave order.
__global__ __launch_bounds__(DDP_REFINE_THREADS) void ddp_refine_energy_kernel(const ddp_refine_args_t A) {
  extern __shared__ float4 tile[];                        // [DDP_REFINE_TILE] (first: 16-byte aligned whatever n is)
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = A.n;
  double* gacc = (double*)(tile + DDP_REFINE_TILE);       // [n][3]
  float* x = (float*)(gacc + 3 * n);                      // [n][3]
  float* rad = x + 3 * n;                                 // [n]
  __shared__ double we[DDP_REFINE_WAVES][3];
  double ec_w, es_w, er_w;
  clash_energy_gradient(A.pos + (size_t)s * n * 3, A.lig_radii, n, A.rec + (size_t)s * A.rec_stride, A.rec_radii, A.m, A.self_pairs,
                        A.anchor + (size_t)s * n * 3, 2.0 * A.overlap, 2.0 * A.restraint / (double)n, tile, gacc, x, rad,
                        A.grad ? A.grad + (size_t)s * n * 3 : nullptr, ec_w, es_w, er_w);
  if (lane == 0) { we[wave][0] = ec_w; we[wave][1] = es_w; we[wave][2] = er_w; }
  __syncthreads();
  if (tid == 0) {
    double ec = we[0][0], es = we[0][1], er = we[0][2];
    for (int w = 1; w < DDP_REFINE_WAVES; ++w) { ec += we[w][0]; es += we[w][1]; er += we[w][2]; }
    er = A.restraint * (er / (double)n);
    double* e = A.energy + 4 * (size_t)s;
    e[0] = ec; e[1] = es; e[2] = er; e[3] = ec + es + er;
  }
}

static int refine_common(const ddp_refine_args_t* a, const char* who, int* rc) {
  // shared shape checks; returns 1 when the call is a no-op or failed (*rc holds the result)
  *rc = 0;
  if (!a) { *rc = ddp_fail(DDP_EINVAL, "ddp_refine: null argument struct"); return 1; }
  if (a->n_samples == 0) return 1;
  if ((*rc = ddp_pose_check_shape(who, a->n_samples, a->n, a->m, a->rec_stride, a->n_tor >= 0))) return 1;
  if ((*rc = DDP_POSE_CHECK_ATOMS(who, a->n, DDP_EVAL_MAX_ATOMS))) return 1;
  return 0;
}

extern "C" int ddp_refine_energy(const ddp_refine_args_t* a, void* stream) {
  int rc;
  if (refine_common(a, "ddp_refine_energy", &rc)) return rc;
  if (!a->pos || !a->anchor || !a->lig_radii || !a->energy || (a->m > 0 && (!a->rec || !a->rec_radii)))
    return ddp_fail(DDP_EINVAL, "ddp_refine_energy: null argument");
  if (!(a->restraint >= 0.0)) return ddp_fail(DDP_EINVAL, "ddp_refine_energy: restraint < 0");
  // the receptor tile + gradient accumulators + ligand coordinates and radii: 16 KiB + 40 n, 56 KiB at the atom limit
  const size_t lds = DDP_REFINE_TILE * sizeof(float4) + (size_t)3 * a->n * sizeof(double) + (size_t)4 * a->n * sizeof(float);
  hipLaunchKernelGGL(ddp_refine_energy_kernel, dim3(a->n_samples), dim3(DDP_REFINE_THREADS), lds, (hipStream_t)stream, *a);
  return ddp_launch_result("ddp_refine_energy");
}

// ---- search direction of sample s: descent_direction (ddp_pose_descent.h) on the pose and the gradient in global memory
__global__ __launch_bounds__(DDP_REFINE_THREADS) void ddp_refine_direction_kernel(const ddp_refine_args_t A) {
  __shared__ double red[DDP_REFINE_WAVES * 6];
  const int s = blockIdx.x, n = A.n, T = A.n_tor;
  descent_direction<false>(A.pos + (size_t)s * n * 3, A.grad + (size_t)s * n * 3, n, T, A.bonds, A.mask_rotate, A.step[s], red, A.tr + 3 * s,
                           A.rot + 3 * s, A.tor + (size_t)s * T);
}

extern "C" int ddp_refine_direction(const ddp_refine_args_t* a, void* stream) {
  int rc;
  if (refine_common(a, "ddp_refine_direction", &rc)) return rc;
  if (!a->pos || !a->grad || !a->step || !a->tr || !a->rot || (a->n_tor > 0 && (!a->tor || !a->bonds || !a->mask_rotate)))
    return ddp_fail(DDP_EINVAL, "ddp_refine_direction: null argument");
  hipLaunchKernelGGL(ddp_refine_direction_kernel, dim3(a->n_samples), dim3(DDP_REFINE_THREADS), 0, (hipStream_t)stream, *a);
  return ddp_launch_result("ddp_refine_direction");
}

// ---- the line search's decision, per sample: trial_energy[s][3] < energy[s][3] (strict, fp64; false for NaN) takes the trial pose,
// its energies and its gradient bit for bit, step = min(grow * step, step_max), accepted += 1; otherwise nothing but step *= shrink
// is written.  Every thread reads the two energies before the barrier, thread 0 overwrites them after it.
__global__ __launch_bounds__(DDP_REFINE_THREADS) void ddp_refine_accept_kernel(const ddp_refine_args_t A) {
  const int s = blockIdx.x, tid = threadIdx.x, n = A.n;
  double* e = A.energy + 4 * (size_t)s;
  const double* et = A.trial_energy + 4 * (size_t)s;
  const bool take = et[3] < e[3];
  __syncthreads();
  if (tid == 0) {
    const double st = A.step[s];
    A.step[s] = take ? fmin(A.grow * st, A.step_max) : A.shrink * st;
    if (take) A.accepted[s] += 1;
  }
  if (!take) return;
  if (tid < 4) e[tid] = et[tid];
  float* x = A.pos + (size_t)s * n * 3;
  const float* xt = A.trial + (size_t)s * n * 3;
  for (int i = tid; i < 3 * n; i += DDP_REFINE_THREADS) x[i] = xt[i];
  if (A.grad && A.trial_grad) {
    double* g = A.grad + (size_t)s * n * 3;
    const double* gt = A.trial_grad + (size_t)s * n * 3;
    for (int i = tid; i < 3 * n; i += DDP_REFINE_THREADS) g[i] = gt[i];
  }
}

extern "C" int ddp_refine_accept(const ddp_refine_args_t* a, void* stream) {
  int rc;
  if (refine_common(a, "ddp_refine_accept", &rc)) return rc;
  if (!a->pos || !a->trial || !a->energy || !a->trial_energy || !a->step || !a->accepted || (!a->grad) != (!a->trial_grad))
    return ddp_fail(DDP_EINVAL, "ddp_refine_accept: null argument");
  hipLaunchKernelGGL(ddp_refine_accept_kernel, dim3(a->n_samples), dim3(DDP_REFINE_THREADS), 0, (hipStream_t)stream, *a);
  return ddp_launch_result("ddp_refine_accept");
}
