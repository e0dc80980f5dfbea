// ddp_score.hip - a Vinardo-form empirical score of sampled poses (include/ddp_hip.h, ddp_pose_score; host side
// diffdock_pocket_amd/scoring.py, which states the whole definition).  The functional form of Vinardo (Quiroga & Villarreal 2016) over
// typed ligand-receptor atom pairs: a gaussian of the surface distance, a quadratic repulsion, a hydrophobic ramp and a hydrogen-bond
// ramp.  Every constant (cutoff, widths, offsets, weights, torsion divisor) comes from the host; only the form is compiled in.  Not
// validated against smina or Vina.
// The launch plan is that of ddp_refine_energy_kernel (csrc/ddp_refine.hip): one 256-thread workgroup per sample, the ligand staged in
// LDS, the receptor streamed through an LDS tile.  The evaluation itself - tile sweep, self pairs, the order of every sum - is
// score_evaluate of ddp_pose_descent.h, which the fused minimiser (ddp_minimize.hip) calls too: this file stages the ligand and packs
// the outputs.  All arithmetic is fp64 on the fp32 inputs (converted first).  No atomics: two launches give the same bits, and a
// sample's result does not depend on the other samples of the launch.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ddp_hip.h"
#include "ddp_internal.h"
#include "ddp_pose_descent.h"

// LDS: the receptor tile (x, y, z, radius) and its flag bytes, the sample's ligand coordinates, radii and flag bytes (fp32 as they
// come), one fp64 gradient accumulator per ligand atom (GRAD only).
template <bool GRAD>
__global__ __launch_bounds__(DDP_DESCENT_THREADS) void ddp_pose_score_kernel(const ddp_score_args_t A) {
  extern __shared__ float4 tile[];                        // [DDP_SCORE_TILE] (first: 16-byte aligned whatever n is)
  const int s = blockIdx.x, tid = threadIdx.x, n = A.n;
  double* gacc = (double*)(tile + DDP_SCORE_TILE);        // [n][3] (GRAD) or nothing
  float* x = (float*)(gacc + (GRAD ? 3 * n : 0));         // [n][3]
  float* rad = x + 3 * n;                                 // [n]
  uint8_t* lflag = (uint8_t*)(rad + n);                   // [n]
  uint8_t* tflag = lflag + n;                             // [DDP_SCORE_TILE]
  __shared__ double we[DDP_DESCENT_WAVES][8];
  const float* __restrict__ ls = A.pos + (size_t)s * n * 3;
  for (int i = tid; i < 3 * n; i += DDP_DESCENT_THREADS) x[i] = ls[i];
  for (int i = tid; i < n; i += DDP_DESCENT_THREADS) { rad[i] = A.lig_radii[i]; lflag[i] = A.lig_flags[i]; }
  score_evaluate<GRAD>(A, A.rec + (size_t)s * A.rec_stride, tile, tflag, x, rad, lflag, gacc, we);
  if (GRAD) {
    double* g = A.grad + (size_t)s * n * 3;
    for (int i = tid; i < 3 * n; i += DDP_DESCENT_THREADS) g[i] = gacc[i];
  }
  if (tid == 0) {
    double t[8], inter, intra;
    score_totals(A.form, we, t, inter, intra);
    double* e = A.energy + 7 * (size_t)s;
    e[0] = t[0]; e[1] = t[1]; e[2] = t[2]; e[3] = t[3]; e[4] = inter; e[5] = intra; e[6] = inter / A.tor_divisor;
  }
}

extern "C" int ddp_pose_score(const ddp_score_args_t* a, void* stream) {
  if (!a) return ddp_fail(DDP_EINVAL, "ddp_pose_score: null argument struct");
  if (a->n_samples == 0) return 0;
  if (const int rc = ddp_pose_check_shape("ddp_pose_score", a->n_samples, a->n, a->m, a->rec_stride, true)) return rc;
  if (const int rc = DDP_POSE_CHECK_ATOMS("ddp_pose_score", a->n, DDP_EVAL_MAX_ATOMS)) return rc;
  if (!a->pos || !a->lig_radii || !a->lig_flags || !a->energy || (a->m > 0 && (!a->rec || !a->rec_radii || !a->rec_flags)))
    return ddp_fail(DDP_EINVAL, "ddp_pose_score: null argument");
  if (const int rc = score_check_constants(&a->form, "ddp_pose_score")) return rc;
  if (!(a->tor_divisor > 0.0)) return ddp_fail(DDP_EINVAL, "ddp_pose_score: tor_divisor must be positive");
  // the receptor tile and its flags + the ligand's coordinates, radii and flags (+ the gradient accumulators): 17 KiB + 17 n (+ 24 n),
  // 58 KiB at the atom limit
  const size_t lds = DDP_SCORE_TILE * (sizeof(float4) + 1) + (size_t)a->n * (4 * sizeof(float) + 1) + (a->grad ? (size_t)3 * a->n * sizeof(double) : 0);
  if (a->grad)
    hipLaunchKernelGGL(ddp_pose_score_kernel<true>, dim3(a->n_samples), dim3(DDP_DESCENT_THREADS), lds, (hipStream_t)stream, *a);
  else
    hipLaunchKernelGGL(ddp_pose_score_kernel<false>, dim3(a->n_samples), dim3(DDP_DESCENT_THREADS), lds, (hipStream_t)stream, *a);
  return ddp_launch_result("ddp_pose_score");
}
