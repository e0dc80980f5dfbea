// ddp_clash_energy.h - the clash energy of one pose and its per-atom gradient, defined once for the clash relief (ddp_refine.hip,
// ddp_refine_energy_kernel) and the guidance term of the reverse-diffusion step (ddp_guidance.hip): the pair term and the pass over
// the receptor and the ligand's own pairs.  One 256-thread workgroup per sample, fp64 on the fp32 inputs (converted first), every sum
// in a fixed order through wave_sum of ddp_pose_descent.h, no atomics.  The LDS carve stays the calling kernel's own.
#ifndef DDP_CLASH_ENERGY_H
#define DDP_CLASH_ENERGY_H
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ddp_pose_descent.h"

#define DDP_REFINE_THREADS DDP_DESCENT_THREADS
#define DDP_REFINE_WAVES DDP_DESCENT_WAVES
#define DDP_REFINE_TILE 1024                     // receptor atoms per LDS tile

// max(0, t - d)^2 of one pair and its gradient with respect to the first atom, added to e and (gx, gy, gz).  The square root is
// taken only where d^2 < t^2 can hold; the comparison is written so that a NaN distance goes through and poisons the sums (a NaN
// energy is never accepted).  d = 0: the energy term counts, the gradient term is zero.
__device__ __forceinline__ void pair_term(double dx, double dy, double dz, double t, double& e, double& gx, double& gy, double& gz) {
  const double d2 = dx * dx + dy * dy + dz * dz;
  if (d2 >= t * t) return;
  const double d = sqrt(d2);
  const double p = t - d;
  if (p <= 0.0) return;
  e += p * p;
  if (d == 0.0) return;
  const double k = -2.0 * p / d;
  gx += k * dx; gy += k * dy; gz += k * dz;
}

// ---- the pass of one sample.  ls [n][3], lig_radii [n]: the pose and the ligand radii in global memory, staged here into x [n][3] and
// rad [n] (LDS, fp32, as ddp_pose_contacts stages them); gacc [n][3]: LDS, one fp64 gradient accumulator per ligand atom; tile: LDS,
// DDP_REFINE_TILE receptor atoms (x, y, z, radius).  The receptor rs [m][3] / rec_radii [m] is streamed through that tile, all 256
// threads loading one tile with coalesced reads: a wave that read the receptor from global memory inside its pair loop waited one L2
// round trip per 64 pairs (measured on 40 poses of 3dpf: 180 us per iteration of the refinement against 125 us with the tile).  Wave
// w owns the ligand atoms i = w, w + 4, ...: for every tile its lanes stride over the tile's atoms, the butterfly gives the tile's
// contribution to atom i, and lane 0 adds it to the atom's accumulator (tiles in increasing order: a fixed order).  Then the lanes
// stride over the ligand atoms j with self_pairs[min(i, j)][max(i, j)] (every self pair is met from both ends and counts half each
// time: exact) and lane 0 adds the restraint term of atom i against anchor `as` [n][3] (global memory or LDS; the pose itself: no
// restraint) with krest = 2 restraint / n.  The gradient of atom i - accumulator + self pairs + restraint, in that order - goes to
// gacc (LDS; visible to the other threads after the caller's next barrier) and, when grad is given, to grad [n][3] in global
// memory.  ec, es, er: this wave's partial sums of E_cross, E_self and sum_i |x_i - anchor_i|^2 over its atoms, in a fixed order (all
// lanes hold the same values); the caller adds them over the waves in wave order.  Called by all 256 threads; x and rad are
// visible to every thread when it returns.
__device__ __forceinline__ void clash_energy_gradient(const float* __restrict__ ls, const float* __restrict__ lig_radii, int n,
                                                      const float* __restrict__ rs, const float* __restrict__ rec_radii, int m,
                                                      const uint8_t* __restrict__ self_pairs, const float* as, double two_ov,
                                                      double krest, float4* tile, double* gacc, float* x, float* rad, double* grad,
                                                      double& ec_w, double& es_w, double& er_w) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i < 3 * n; i += DDP_REFINE_THREADS) { x[i] = ls[i]; gacc[i] = 0.0; }
  for (int i = tid; i < n; i += DDP_REFINE_THREADS) rad[i] = lig_radii[i];
  ec_w = 0.0; es_w = 0.0; er_w = 0.0;
  for (int j0 = 0; j0 < m; j0 += DDP_REFINE_TILE) {
    const int mt = min(DDP_REFINE_TILE, m - j0);
    __syncthreads();                             // the previous tile has been used (first pass: x, rad, gacc are visible)
    for (int j = tid; j < mt; j += DDP_REFINE_THREADS)
      tile[j] = make_float4(rs[3 * (j0 + j)], rs[3 * (j0 + j) + 1], rs[3 * (j0 + j) + 2], rec_radii[j0 + j]);
    __syncthreads();
    for (int i = wave; i < n; i += DDP_REFINE_WAVES) {
      const double xi = x[3 * i], yi = x[3 * i + 1], zi = x[3 * i + 2], ri = rad[i];
      double ec = 0.0, gx = 0.0, gy = 0.0, gz = 0.0;
      for (int j = lane; j < mt; j += 64) {
        const float4 r = tile[j];
        if (r.w < 0.f) continue;                 // a receptor hydrogen
        const double t = ri + (double)r.w - two_ov;
        if (t <= 0.0) continue;
        pair_term(xi - (double)r.x, yi - (double)r.y, zi - (double)r.z, t, ec, gx, gy, gz);
      }
      ec = wave_sum(ec); gx = wave_sum(gx); gy = wave_sum(gy); gz = wave_sum(gz);
      ec_w += ec;
      if (lane == 0) { gacc[3 * i] += gx; gacc[3 * i + 1] += gy; gacc[3 * i + 2] += gz; }   // (atom i is this wave's alone)
    }
  }
  __syncthreads();                               // m = 0: x and rad are visible
  for (int i = wave; i < n; i += DDP_REFINE_WAVES) {
    const double xi = x[3 * i], yi = x[3 * i + 1], zi = x[3 * i + 2], ri = rad[i];
    double es = 0.0, gx = 0.0, gy = 0.0, gz = 0.0;
    if (self_pairs) {
      for (int j = lane; j < n; j += 64) {
        if (j == i || !self_pairs[(size_t)min(i, j) * n + max(i, j)]) continue;
        const double t = ri + (double)rad[j] - two_ov;
        if (t <= 0.0) continue;
        pair_term(xi - (double)x[3 * j], yi - (double)x[3 * j + 1], zi - (double)x[3 * j + 2], t, es, gx, gy, gz);
      }
      es = wave_sum(es); gx = wave_sum(gx); gy = wave_sum(gy); gz = wave_sum(gz);
    }
    const double ax = xi - (double)as[3 * i], ay = yi - (double)as[3 * i + 1], az = zi - (double)as[3 * i + 2];
    es_w += 0.5 * es; er_w += ax * ax + ay * ay + az * az;
    if (lane == 0) {
      const double g0 = gacc[3 * i] + gx + krest * ax, g1 = gacc[3 * i + 1] + gy + krest * ay, g2 = gacc[3 * i + 2] + gz + krest * az;
      gacc[3 * i] = g0; gacc[3 * i + 1] = g1; gacc[3 * i + 2] = g2;
      if (grad) { grad[3 * i] = g0; grad[3 * i + 1] = g1; grad[3 * i + 2] = g2; }
    }
  }
}

#endif
