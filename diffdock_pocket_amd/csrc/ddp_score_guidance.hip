// ddp_score_guidance.hip - the physics-score guidance term of the reverse-diffusion step (include/ddp_hip.h, ddp_score_guidance; host
// side diffdock_pocket_amd/score_guidance.py and sampler.py).  This project's own term, not part of the reference.  Between
// ddp_sde_update (ddp_svgd_rows and ddp_clash_guidance, where they run) and ddp_pose_update, the updates of every sample are nudged
// down the gradient of the Vinardo-form score of ddp_score.hip, along the sampler's own degrees of freedom.  For sample s with the fp32
// pose x the scores were computed for and g = dE/dx the fp64 gradient of E = inter + intra (the minimiser's energy at restraint 0, not
// divided by the torsion divisor):
//   1. w = *weight: one fp32 value in device memory, the step's w_t (score_guidance_weight while t <= score_guidance_t_max, else 0).
//      A per-step constant, not multiplied by g^2 dt: more steps mean more total guidance.  Unless w > 0 nothing is stored.
//   2. (d_tr, d_rot, d_tor) = descent_direction(x, g, step = w), rounded to fp32: what ddp_refine_direction writes for step[s] = w.
//   3. f_s = min(1, max_tr / |d_tr|_2, max_rot / |d_rot|_2, max_tor / max_b |d_tor[b]|) in fp64 from those fp32 values; a zero norm
//      contributes no constraint.
//   4. upd_X[s] += (float)(f_s * (double)d_X) for X in tr, rot, tor; every element by one thread, no atomics.
// One launch, one 256-thread workgroup per sample, the shape of ddp_clash_guidance_kernel: score_evaluate<true> of ddp_pose_descent.h
// leaves the gradient in LDS, descent_direction reads the pose and the gradient there and leaves the direction in LDS, the cap factor
// comes from one more block reduction (a maximum: the order does not matter), then the read-modify-write of upd.  Every sum has a
// fixed order: two launches give the same bits.  A NaN pose poisons its own sample only (no value crosses workgroups).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ddp_hip.h"
#include "ddp_internal.h"
#include "ddp_pose_descent.h"

// The dynamic LDS, in the order of the carve below.  fp64 follows the tile (every offset a multiple of 8 bytes: the tile starts the
// region, 16-byte aligned), then fp32, then the flag bytes.
#define SG_FP64(n) ((size_t)3 * (n) + DDP_DESCENT_WAVES * 6 + DDP_DESCENT_WAVES * 8)      /* gradient, red, we */
#define SG_FP32(n, n_tor) ((size_t)4 * (n) + (n_tor) + 8)                                 /* pose, radii, torsion steps, d_tr and d_rot */
#define SG_BYTES(n) ((size_t)(n) + DDP_SCORE_TILE)                                        /* ligand flags, tile flags */
#define SG_LDS_BYTES(n, n_tor) \
  (DDP_SCORE_TILE * sizeof(float4) + SG_FP64(n) * sizeof(double) + SG_FP32(n, n_tor) * sizeof(float) + SG_BYTES(n))
// 17 KiB + 41 n + 4 n_tor + 480 bytes: 63968 bytes (62.5 KiB) at both limits
static_assert(SG_LDS_BYTES(DDP_EVAL_MAX_ATOMS, DDP_GUIDANCE_MAX_TORSIONS) <= 64 * 1024,
              "ddp_score_guidance: the LDS plan must fit the 64 KiB a workgroup gets without opting in to more");

__global__ __launch_bounds__(DDP_DESCENT_THREADS) void ddp_score_guidance_kernel(const ddp_score_guidance_args_t A) {
  const float w = *A.weight;
  if (!(w > 0.f)) return;                                 // (the same for all threads and all workgroups) nothing is stored
  extern __shared__ float4 tile[];                        // [DDP_SCORE_TILE]
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = A.n, T = A.n_tor;
  double* gacc = (double*)(tile + DDP_SCORE_TILE);        // [n][3]
  double* red = gacc + 3 * n;                             // [waves][6]
  double (*we)[8] = (double (*)[8])(red + DDP_DESCENT_WAVES * 6);   // [waves][8]
  float* x = (float*)(we + DDP_DESCENT_WAVES);            // [n][3]
  float* rad = x + 3 * n;                                 // [n]
  float* tor = rad + n;                                   // [T]
  float* dir = tor + T;                                   // d_tr [3], d_rot [3] (+ 2 unused)
  uint8_t* lflag = (uint8_t*)(dir + 8);                   // [n]
  uint8_t* tflag = lflag + n;                             // [DDP_SCORE_TILE]
  const float* __restrict__ ls = A.pos + (size_t)s * n * 3;
  for (int i = tid; i < 3 * n; i += DDP_DESCENT_THREADS) x[i] = ls[i];
  for (int i = tid; i < n; i += DDP_DESCENT_THREADS) { rad[i] = A.lig_radii[i]; lflag[i] = A.lig_flags[i]; }
  score_evaluate<true>(A, A.rec + (size_t)s * A.rec_stride, tile, tflag, x, rad, lflag, gacc, we);   // ends with a barrier
  if (A.grad) {
    double* g = A.grad + (size_t)s * n * 3;
    for (int i = tid; i < 3 * n; i += DDP_DESCENT_THREADS) g[i] = gacc[i];
  }
  if (A.energy && tid == 0) {
    double t[8], inter, intra;
    score_totals(A.form, we, t, inter, intra);
    A.energy[2 * (size_t)s] = inter; A.energy[2 * (size_t)s + 1] = intra;
  }
  descent_direction<false>(x, gacc, n, T, A.bonds, A.mask_rotate, (double)w, red, dir, dir + 3, tor);
  __syncthreads();                                        // dir (thread 0) and tor (lane 0 of the owning waves) are visible
  double mx = 0.0;
  for (int b = tid; b < T; b += DDP_DESCENT_THREADS) mx = fmax(mx, fabs((double)tor[b]));
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) mx = fmax(mx, __shfl_xor(mx, off));
  if (lane == 0) red[wave] = mx;                          // (red's last readers passed the barrier above)
  __syncthreads();
  mx = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
  const double tx = dir[0], ty = dir[1], tz = dir[2], rx = dir[3], ry = dir[4], rz = dir[5];
  const double nt = sqrt(tx * tx + ty * ty + tz * tz), nr = sqrt(rx * rx + ry * ry + rz * rz);
  double f = 1.0;
  if (nt > 0.0) f = fmin(f, A.max_tr / nt);
  if (nr > 0.0) f = fmin(f, A.max_rot / nr);
  if (mx > 0.0) f = fmin(f, A.max_tor / mx);
  if (tid < 6) {
    float* u = A.upd[tid / 3] + 3 * (size_t)s + tid % 3;
    *u = *u + (float)(f * (double)dir[tid]);
  }
  if (T > 0) {
    float* u = A.upd[2] + (size_t)s * T;
    for (int b = tid; b < T; b += DDP_DESCENT_THREADS) u[b] = u[b] + (float)(f * (double)tor[b]);
  }
}

extern "C" int ddp_score_guidance(const ddp_score_guidance_args_t* a, void* stream) {
  if (!a) return ddp_fail(DDP_EINVAL, "ddp_score_guidance: null argument struct");
  if (a->n_samples == 0) return 0;
  if (const int rc = ddp_pose_check_shape("ddp_score_guidance", a->n_samples, a->n, a->m, a->rec_stride, a->n_tor >= 0)) return rc;
  if (const int rc = DDP_POSE_CHECK_ATOMS("ddp_score_guidance", a->n, DDP_EVAL_MAX_ATOMS)) return rc;
  if (a->n_tor > DDP_GUIDANCE_MAX_TORSIONS) return ddp_fail(DDP_ELIMIT, "ddp_score_guidance: more than DDP_GUIDANCE_MAX_TORSIONS rotatable bonds");
  if (!a->pos || !a->lig_radii || !a->lig_flags || !a->weight || !a->upd[0] || !a->upd[1] ||
      (a->m > 0 && (!a->rec || !a->rec_radii || !a->rec_flags)) || (a->n_tor > 0 && (!a->bonds || !a->mask_rotate || !a->upd[2])))
    return ddp_fail(DDP_EINVAL, "ddp_score_guidance: null argument");
  if (const int rc = score_check_constants(&a->form, "ddp_score_guidance")) return rc;
  if (!(a->max_tr >= 0.0) || !(a->max_rot >= 0.0) || !(a->max_tor >= 0.0))
    return ddp_fail(DDP_EINVAL, "ddp_score_guidance: the caps must not be negative or NaN");
  hipLaunchKernelGGL(ddp_score_guidance_kernel, dim3(a->n_samples), dim3(DDP_DESCENT_THREADS), SG_LDS_BYTES(a->n, a->n_tor),
                     (hipStream_t)stream, *a);
  return ddp_launch_result("ddp_score_guidance");
}
