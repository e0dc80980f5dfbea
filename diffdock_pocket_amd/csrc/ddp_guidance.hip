// ddp_guidance.hip - the steric-clash guidance term of the reverse-diffusion step (include/ddp_hip.h, ddp_clash_guidance; host side
// diffdock_pocket_amd/guidance.py and sampler.py).  This project's own term, not part of the reference.  Between ddp_sde_update (and
// ddp_svgd_rows) and ddp_pose_update, the updates of every sample are nudged down the gradient of the clash energy of ddp_refine.hip,
// along the sampler's own degrees of freedom.  For sample s with the fp32 pose x the scores were computed for and g = dE/dx the fp64
// gradient of E = E_cross + E_self (restraint 0, receptor hydrogens ignored):
//   1. w = *weight: one fp32 value in device memory, the step's w_t (clash_guidance_weight while t <= clash_guidance_t_max, else 0).
//      A per-step constant, not multiplied by g^2 dt: more steps mean more total guidance.  Unless w > 0 nothing is stored.
//   2. (d_tr, d_rot, d_tor) = descent_direction(x, g, step = w), rounded to fp32: what ddp_refine_direction writes for step[s] = w.
//   3. f_s = min(1, max_tr / |d_tr|_2, max_rot / |d_rot|_2, max_tor / max_b |d_tor[b]|) in fp64 from those fp32 values; a zero norm
//      contributes no constraint.
//   4. upd_X[s] += (float)(f_s * (double)d_X) for X in tr, rot, tor; every element by one thread, no atomics.
// One launch, one 256-thread workgroup per sample: the energy pass of ddp_clash_energy.h leaves the gradient in LDS, descent_direction
// of ddp_pose_descent.h reads the pose and the gradient there and leaves the direction in LDS, the cap factor comes from one more
// block reduction (a maximum: the order does not matter), then the read-modify-write of upd.  Every sum has a fixed order: two
// launches give the same bits.  A NaN pose poisons its own sample only (no value crosses workgroups).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ddp_hip.h"
#include "ddp_internal.h"
#include "ddp_clash_energy.h"
#include "ddp_pose_descent.h"

// floats of the dynamic LDS after the tile: fp64 first (the gradient, the reductions' scratch red [waves][6], the energy partials we
// [waves][2]), then fp32 (pose, radii, torsion components, d_tr and d_rot).  Every fp64 offset is a multiple of 8 bytes, the tile
// starts the region: 16-byte aligned.
static size_t guidance_lds_bytes(int n, int n_tor) {
  return DDP_REFINE_TILE * sizeof(float4) + ((size_t)3 * n + DDP_REFINE_WAVES * 6 + DDP_REFINE_WAVES * 2) * sizeof(double) +
         ((size_t)4 * n + n_tor + 8) * sizeof(float);
}

__global__ __launch_bounds__(DDP_REFINE_THREADS) void ddp_clash_guidance_kernel(const ddp_clash_guidance_args_t A) {
  const float w = *A.weight;
  if (!(w > 0.f)) return;                                 // (the same for all threads and all workgroups) nothing is stored
  extern __shared__ float4 tile[];                        // [DDP_REFINE_TILE]
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = A.n, T = A.n_tor;
  double* gacc = (double*)(tile + DDP_REFINE_TILE);       // [n][3]
  double* red = gacc + 3 * n;                             // [waves][6]
  double* we = red + DDP_REFINE_WAVES * 6;                // [waves][2]
  float* x = (float*)(we + DDP_REFINE_WAVES * 2);         // [n][3]
  float* rad = x + 3 * n;                                 // [n]
  float* tor = rad + n;                                   // [T]
  float* dir = tor + T;                                   // d_tr [3], d_rot [3]
  double ec_w, es_w, er_w;
  // anchor = the staged pose itself: the restraint terms are x - x = 0 (NaN for a NaN coordinate, as ddp_refine_energy with anchor = pos)
  clash_energy_gradient(A.pos + (size_t)s * n * 3, A.lig_radii, n, A.rec + (size_t)s * A.rec_stride, A.rec_radii, A.m, A.self_pairs, x,
                        2.0 * A.overlap, 0.0, tile, gacc, x, rad, A.grad ? A.grad + (size_t)s * n * 3 : nullptr, ec_w, es_w, er_w);
  if (lane == 0) { we[2 * wave] = ec_w; we[2 * wave + 1] = es_w; }
  __syncthreads();                                        // the gradient in gacc and the partials are visible
  if (A.energy && tid == 0) {
    double ec = we[0], es = we[1];
    for (int k = 1; k < DDP_REFINE_WAVES; ++k) { ec += we[2 * k]; es += we[2 * k + 1]; }
    A.energy[2 * (size_t)s] = ec; A.energy[2 * (size_t)s + 1] = es;
  }
  descent_direction<false>(x, gacc, n, T, A.bonds, A.mask_rotate, (double)w, red, dir, dir + 3, tor);
  __syncthreads();                                        // dir (thread 0) and tor (lane 0 of the owning waves) are visible
  double mx = 0.0;
  for (int b = tid; b < T; b += DDP_REFINE_THREADS) mx = fmax(mx, fabs((double)tor[b]));
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
    for (int b = tid; b < T; b += DDP_REFINE_THREADS) u[b] = u[b] + (float)(f * (double)tor[b]);
  }
}

extern "C" int ddp_clash_guidance(const ddp_clash_guidance_args_t* a, void* stream) {
  if (!a) return ddp_fail(DDP_EINVAL, "ddp_clash_guidance: null argument struct");
  if (a->n_samples == 0) return 0;
  if (const int rc = ddp_pose_check_shape("ddp_clash_guidance", a->n_samples, a->n, a->m, a->rec_stride, a->n_tor >= 0)) return rc;
  if (const int rc = DDP_POSE_CHECK_ATOMS("ddp_clash_guidance", a->n, DDP_EVAL_MAX_ATOMS)) return rc;
  if (a->n_tor > DDP_GUIDANCE_MAX_TORSIONS) return ddp_fail(DDP_ELIMIT, "ddp_clash_guidance: more than DDP_GUIDANCE_MAX_TORSIONS rotatable bonds");
  if (!a->pos || !a->lig_radii || !a->weight || !a->upd[0] || !a->upd[1] || (a->m > 0 && (!a->rec || !a->rec_radii)) ||
      (a->n_tor > 0 && (!a->bonds || !a->mask_rotate || !a->upd[2])))
    return ddp_fail(DDP_EINVAL, "ddp_clash_guidance: null argument");
  if (!(a->max_tr >= 0.0) || !(a->max_rot >= 0.0) || !(a->max_tor >= 0.0) || !isfinite(a->overlap))
    return ddp_fail(DDP_EINVAL, "ddp_clash_guidance: the caps must not be negative or NaN, overlap must be finite");
  // 16 KiB + 40 n + 4 n_tor + 288 bytes: 60.3 KiB at both limits, under the 64 KiB a workgroup gets without opting in to more
  hipLaunchKernelGGL(ddp_clash_guidance_kernel, dim3(a->n_samples), dim3(DDP_REFINE_THREADS), guidance_lds_bytes(a->n, a->n_tor),
                     (hipStream_t)stream, *a);
  return ddp_launch_result("ddp_clash_guidance");
}
