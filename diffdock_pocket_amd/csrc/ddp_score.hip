// ddp_score.hip - a Vinardo-form empirical score of sampled poses (include/ddp_hip.h, ddp_pose_score; host side
// diffdock_pocket_amd/scoring.py, which states the whole definition).  The functional form of Vinardo (Quiroga & Villarreal 2016) over
// typed ligand-receptor atom pairs: a gaussian of the surface distance, a quadratic repulsion, a hydrophobic ramp and a hydrogen-bond
// ramp.  Every constant (cutoff, widths, offsets, weights, torsion divisor) comes from the host; only the form is compiled in.  Not
// validated against smina or Vina.
// The launch plan is that of ddp_refine_energy_kernel (csrc/ddp_refine.hip): one 256-thread workgroup per sample, the ligand staged in
// LDS, the receptor streamed through a tile of DDP_SCORE_TILE atoms that all 256 threads load with coalesced reads (that file records
// why: a wave that reads the receptor from global memory inside its pair loop waits one L2 round trip per 64 pairs).  Wave w owns the
// ligand atoms i = w, w + 4, ...; its lanes stride over the tile.  The energy sums stay in lane-private accumulators over all the
// atoms and tiles a lane meets (a fixed sequence) and go through one __shfl_xor butterfly at the end, the waves are then added in wave
// order; the gradient of atom i goes through the butterfly once per tile and lane 0 adds it to the atom's accumulator (tiles in
// increasing order).  All arithmetic is fp64 on the fp32 inputs (converted first).  No atomics: two launches give the same bits, and
// a sample's result does not depend on the other samples of the launch.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ddp_hip.h"
#include "ddp_internal.h"
#include "ddp_score_pair.h"

#define DDP_SCORE_THREADS 256
#define DDP_SCORE_WAVES (DDP_SCORE_THREADS / 64)
#define DDP_SCORE_TILE 1024

// score_wave_sum, ScoreAcc and score_pair live in ddp_score_pair.h (shared with ddp_minimize.hip)

// LDS: the receptor tile (x, y, z, radius) and its flag bytes, the sample's ligand coordinates, radii and flag bytes (fp32 as they
// come), one fp64 gradient accumulator per ligand atom (GRAD only).
template <bool GRAD>
__global__ __launch_bounds__(DDP_SCORE_THREADS) void ddp_pose_score_kernel(const ddp_score_args_t A) {
  extern __shared__ float4 tile[];                        // [DDP_SCORE_TILE] (first: 16-byte aligned whatever n is)
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = A.n, m = A.m;
  double* gacc = (double*)(tile + DDP_SCORE_TILE);        // [n][3] (GRAD) or nothing
  float* x = (float*)(gacc + (GRAD ? 3 * n : 0));         // [n][3]
  float* rad = x + 3 * n;                                 // [n]
  uint8_t* lflag = (uint8_t*)(rad + n);                   // [n]
  uint8_t* tflag = lflag + n;                             // [DDP_SCORE_TILE]
  __shared__ double we[DDP_SCORE_WAVES][8];
  const float* __restrict__ ls = A.pos + (size_t)s * n * 3;
  const float* __restrict__ rs = A.rec + (size_t)s * A.rec_stride;
  for (int i = tid; i < 3 * n; i += DDP_SCORE_THREADS) {
    x[i] = ls[i];
    if (GRAD) gacc[i] = 0.0;
  }
  for (int i = tid; i < n; i += DDP_SCORE_THREADS) { rad[i] = A.lig_radii[i]; lflag[i] = A.lig_flags[i]; }
  const double cut2 = A.cutoff * A.cutoff;
  ScoreAcc cross = {{0.0, 0.0, 0.0, 0.0}, 0.0, 0.0, 0.0};  // this lane's share, over every atom and tile it meets
  for (int j0 = 0; j0 < m; j0 += DDP_SCORE_TILE) {
    const int mt = min(DDP_SCORE_TILE, m - j0);
    __syncthreads();                             // the previous tile has been used (first pass: the ligand is visible)
    for (int j = tid; j < mt; j += DDP_SCORE_THREADS) {
      tile[j] = make_float4(rs[3 * (j0 + j)], rs[3 * (j0 + j) + 1], rs[3 * (j0 + j) + 2], A.rec_radii[j0 + j]);
      tflag[j] = A.rec_flags[j0 + j];
    }
    __syncthreads();
    for (int i = wave; i < n; i += DDP_SCORE_WAVES) {
      const double ri = rad[i];
      if (ri < 0.0) continue;                    // an untyped ligand atom (wave-uniform)
      const double xi = x[3 * i], yi = x[3 * i + 1], zi = x[3 * i + 2];
      const unsigned fi = lflag[i];
      cross.gx = cross.gy = cross.gz = 0.0;
      for (int j = lane; j < mt; j += 64) {
        const float4 r = tile[j];
        if (r.w < 0.f) continue;                 // an untyped receptor atom
        score_pair<GRAD>(A, cut2, xi - (double)r.x, yi - (double)r.y, zi - (double)r.z, ri + (double)r.w, fi, tflag[j], cross);
      }
      if (GRAD) {
        const double gx = score_wave_sum(cross.gx), gy = score_wave_sum(cross.gy), gz = score_wave_sum(cross.gz);
        if (lane == 0) { gacc[3 * i] += gx; gacc[3 * i + 1] += gy; gacc[3 * i + 2] += gz; }   // (atom i is this wave's alone)
      }
    }
  }
  __syncthreads();                               // m = 0: the ligand is visible
  ScoreAcc self = {{0.0, 0.0, 0.0, 0.0}, 0.0, 0.0, 0.0};
  for (int i = wave; i < n; i += DDP_SCORE_WAVES) {
    const double ri = rad[i];
    self.gx = self.gy = self.gz = 0.0;
    if (A.self_pairs && ri >= 0.0) {
      const double xi = x[3 * i], yi = x[3 * i + 1], zi = x[3 * i + 2];
      const unsigned fi = lflag[i];
      for (int j = lane; j < n; j += 64) {
        if (j == i || rad[j] < 0.f || !A.self_pairs[(size_t)min(i, j) * n + max(i, j)]) continue;
        score_pair<GRAD>(A, cut2, xi - (double)x[3 * j], yi - (double)x[3 * j + 1], zi - (double)x[3 * j + 2], ri + (double)rad[j], fi,
                         lflag[j], self);
      }
    }
    if (GRAD) {
      const double gx = score_wave_sum(self.gx), gy = score_wave_sum(self.gy), gz = score_wave_sum(self.gz);
      if (lane == 0) {
        double* g = A.grad + ((size_t)s * n + i) * 3;
        g[0] = gacc[3 * i] + gx; g[1] = gacc[3 * i + 1] + gy; g[2] = gacc[3 * i + 2] + gz;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double c = score_wave_sum(cross.t[k]), f = score_wave_sum(self.t[k]);
    if (lane == 0) { we[wave][k] = c; we[wave][4 + k] = f; }
  }
  __syncthreads();
  if (tid == 0) {
    double t[8];
    for (int k = 0; k < 8; ++k) {
      t[k] = we[0][k];
      for (int w = 1; w < DDP_SCORE_WAVES; ++w) t[k] += we[w][k];
    }
    const double inter = A.w_gauss * t[0] + A.w_repulsion * t[1] + A.w_hydrophobic * t[2] + A.w_hbond * t[3];
    // every self pair is met from both ends and counts half each time: exact
    const double intra = A.w_gauss * (0.5 * t[4]) + A.w_repulsion * (0.5 * t[5]) + A.w_hydrophobic * (0.5 * t[6]) + A.w_hbond * (0.5 * t[7]);
    double* e = A.energy + 7 * (size_t)s;
    e[0] = t[0]; e[1] = t[1]; e[2] = t[2]; e[3] = t[3]; e[4] = inter; e[5] = intra; e[6] = inter / A.tor_divisor;
  }
}

extern "C" int ddp_pose_score(const ddp_score_args_t* a, void* stream) {
  if (!a) return ddp_fail(DDP_EINVAL, "ddp_pose_score: null argument struct");
  if (a->n_samples == 0) return 0;
  if (a->n_samples < 0 || a->n <= 0 || a->m < 0 || (a->rec_stride != 0 && a->rec_stride < 3 * a->m))
    return ddp_fail(DDP_EINVAL, "ddp_pose_score: shape");
  if (a->n > DDP_EVAL_MAX_ATOMS) return ddp_fail(DDP_ELIMIT, "ddp_pose_score: more than DDP_EVAL_MAX_ATOMS ligand atoms");
  if (!a->pos || !a->lig_radii || !a->lig_flags || !a->energy || (a->m > 0 && (!a->rec || !a->rec_radii || !a->rec_flags)))
    return ddp_fail(DDP_EINVAL, "ddp_pose_score: null argument");
  if (!(a->cutoff > 0.0) || !isfinite(a->cutoff)) return ddp_fail(DDP_EINVAL, "ddp_pose_score: cutoff must be positive and finite");
  if (!(a->gauss_width > 0.0) || !(a->hydrophobic_bad > a->hydrophobic_good) || !(a->hbond_bad > a->hbond_good) || !(a->tor_divisor > 0.0))
    return ddp_fail(DDP_EINVAL, "ddp_pose_score: gauss_width and tor_divisor must be positive, every ramp must have good < bad");
  // the receptor tile and its flags + the ligand's coordinates, radii and flags (+ the gradient accumulators): 17 KiB + 17 n (+ 24 n),
  // 58 KiB at the atom limit
  const size_t lds = DDP_SCORE_TILE * (sizeof(float4) + 1) + (size_t)a->n * (4 * sizeof(float) + 1) + (a->grad ? (size_t)3 * a->n * sizeof(double) : 0);
  if (a->grad)
    hipLaunchKernelGGL(ddp_pose_score_kernel<true>, dim3(a->n_samples), dim3(DDP_SCORE_THREADS), lds, (hipStream_t)stream, *a);
  else
    hipLaunchKernelGGL(ddp_pose_score_kernel<false>, dim3(a->n_samples), dim3(DDP_SCORE_THREADS), lds, (hipStream_t)stream, *a);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return ddp_fail_hip(err, "ddp_pose_score launch");
  return 0;
}
