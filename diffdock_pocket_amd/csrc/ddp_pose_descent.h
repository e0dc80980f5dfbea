// ddp_pose_descent.h - the pieces that the clash relief (ddp_refine.hip), the physics score (ddp_score.hip), the two minimisers
// (ddp_minimize.hip, ddp_minimize_flex.hip), the two searches (ddp_search.hip, ddp_search_flex.hip) and the three guidance terms
// (ddp_guidance.hip, ddp_score_guidance.hip, ddp_score_guidance_flex.hip) share, each defined once: the fixed-order reductions, the
// search direction in pose space, the pose map on a pose held in LDS, the evaluation of the Vinardo-form score, the ligand restraint
// pass.  All of them run one 256-thread workgroup per sample.  Every function
// takes plain pointers (global memory or LDS:
// the callers are inlined, so the compiler sees the address space) and the LDS carve stays the calling kernel's own.  Every sum has a
// fixed order: a wave owns an output (a ligand atom, a rotatable bond), its 64 lanes stride over the summands, a butterfly of
// __shfl_xor (every stage adds two equal-rank partial sums, addition is commutative: all lanes end with the same bits), and sums over
// waves run in wave order.  No atomics: two launches give the same bits.
#ifndef DDP_POSE_DESCENT_H
#define DDP_POSE_DESCENT_H
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "ddp_internal.h"
#include "ddp_horn.h"
#include "ddp_score_pair.h"

#define DDP_DESCENT_THREADS 256
#define DDP_DESCENT_WAVES (DDP_DESCENT_THREADS / 64)
#define DDP_SCORE_TILE 1024                      // receptor atoms per LDS tile of score_evaluate

template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// block sum of K values, all threads get the result: butterfly, then the waves in wave order.  red: LDS, [waves][K].  Two barriers:
// the first frees `red` of the previous sum's readers, the second publishes this one.
template <typename T, int K>
__device__ __forceinline__ void block_sum(T* v, T* red, int lane, int wave) {
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = wave_sum(v[k]);
  __syncthreads();
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) red[wave * K + k] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) {
    T acc = red[k];
    for (int w = 1; w < DDP_DESCENT_WAVES; ++w) acc += red[w * K + k];
    v[k] = acc;
  }
}

// ---- search direction of one sample, each degree of freedom scaled by its unit-mass inertia and multiplied by step:
//   tr = -sum g_i / n,   rot = -sum (x_i - c) x g_i / sum |x_i - c|^2,   tor[b] = -sum g_i . a_i / sum |a_i|^2 over mask_rotate[b],
//   a_i = u^ x (x_i - x_v), u^ = (x_u - x_v) / |x_u - x_v| (axis and sense of ddp_pose_update; atoms u and v themselves are left out of
//   the sums: their lever is zero); a zero denominator gives 0.  fp64 on the fp32 pose x [n][3] and the gradient g [n][3], rounded to
//   fp32 at the end.  tr[3] and rot[3] are written by every thread (EVERY_THREAD: the caller hands in registers and every thread
//   goes on with the steps, as the fused minimiser does) or by thread 0 alone (memory, as ddp_refine_direction_kernel hands in; there
//   the divisions of all threads would cost 32 VGPRs and three of eight waves per SIMD).  tor[b] is written by lane 0 of the wave that
//   owns bond b = w, w + 4, ...: global memory or LDS, visible to the other threads after the caller's next barrier.  red: LDS, 4 * 6
//   doubles.
template <bool EVERY_THREAD>
__device__ __forceinline__ void descent_direction(const float* __restrict__ x, const double* __restrict__ g, int n, int T,
                                                  const int32_t* __restrict__ bonds, const uint8_t* __restrict__ mask_rotate, double step,
                                                  double* red, float* tr, float* rot, float* tor) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int i = tid; i < n; i += DDP_DESCENT_THREADS) {
    v[0] += (double)x[3 * i]; v[1] += (double)x[3 * i + 1]; v[2] += (double)x[3 * i + 2];
    v[3] += g[3 * i]; v[4] += g[3 * i + 1]; v[5] += g[3 * i + 2];
  }
  block_sum<double, 6>(v, red, lane, wave);
  const double cx = v[0] / n, cy = v[1] / n, cz = v[2] / n;
  if (EVERY_THREAD || tid == 0) {
    tr[0] = (float)(step * (-v[3] / n)); tr[1] = (float)(step * (-v[4] / n)); tr[2] = (float)(step * (-v[5] / n));
  }
  double r[4] = {0.0, 0.0, 0.0, 0.0};
  for (int i = tid; i < n; i += DDP_DESCENT_THREADS) {
    const double px = (double)x[3 * i] - cx, py = (double)x[3 * i + 1] - cy, pz = (double)x[3 * i + 2] - cz;
    const double gx = g[3 * i], gy = g[3 * i + 1], gz = g[3 * i + 2];
    r[0] += py * gz - pz * gy; r[1] += pz * gx - px * gz; r[2] += px * gy - py * gx;
    r[3] += px * px + py * py + pz * pz;
  }
  block_sum<double, 4>(r, red, lane, wave);
  if (EVERY_THREAD || tid == 0) {
    for (int k = 0; k < 3; ++k) rot[k] = (float)(step * (r[3] == 0.0 ? 0.0 : -r[k] / r[3]));
  }
  for (int b = wave; b < T; b += DDP_DESCENT_WAVES) {
    const int u = bonds[2 * b], w = bonds[2 * b + 1];
    double num = 0.0, den = 0.0;
    if (u >= 0 && u < n && w >= 0 && w < n) {    // an entry outside the ligand: no read, the bond gets 0
      const double vx = x[3 * w], vy = x[3 * w + 1], vz = x[3 * w + 2];
      double ux = (double)x[3 * u] - vx, uy = (double)x[3 * u + 1] - vy, uz = (double)x[3 * u + 2] - vz;
      const double len = sqrt(ux * ux + uy * uy + uz * uz);
      ux /= len; uy /= len; uz /= len;
      const uint8_t* __restrict__ mk = mask_rotate + (size_t)b * n;
      for (int i = lane; i < n; i += 64) {
        if (!mk[i] || i == u || i == w) continue;  // the bond's own atoms lie on the axis: no lever, exactly
        const double px = (double)x[3 * i] - vx, py = (double)x[3 * i + 1] - vy, pz = (double)x[3 * i + 2] - vz;
        const double ax = uy * pz - uz * py, ay = uz * px - ux * pz, az = ux * py - uy * px;
        num += g[3 * i] * ax + g[3 * i + 1] * ay + g[3 * i + 2] * az;
        den += ax * ax + ay * ay + az * az;
      }
    }
    num = wave_sum(num); den = wave_sum(den);
    if (lane == 0) tor[b] = (float)(step * (den == 0.0 ? 0.0 : -num / den));
  }
}

// ---- xt = the pose map of ddp_pose_update_kernel applied to x with (tr, rot, tor), fp32, on a pose held in LDS: the rigid move about the
// centroid, the torsions in bond order, the Horn re-alignment through ddp_horn.h (every thread runs the 4x4 Jacobi on the same block
// sums: the same bits in every thread, and no barrier to publish a matrix).  A: the kernel's arguments (n, n_tor, bonds, mask_rotate);
// rg [n][3]: LDS, receives the rigid copy; tor [n_tor]: the torsion steps, LDS, visible on entry; redf: LDS scratch of block_sum, at
// least [waves][9] floats.  Called by all 256 threads; ends with a barrier: xt is visible on return.  Shared by the fused minimiser
// (ddp_minimize.hip) and the joint minimiser (ddp_minimize_flex.hip).
template <class Args>
__device__ __forceinline__ void descent_pose_update(const Args& A, const float* x, float* xt, float* rg, const float* tor, float* redf,
                                                    const float* tr, const float* rot) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = A.n, T = A.n_tor;
  const float inv_n = 1.0f / (float)n;
  float M[9];
  // rigid move about the centre: (x - c) R^T + tr + c
  float c[3] = {0.f, 0.f, 0.f};
  for (int i = tid; i < n; i += DDP_DESCENT_THREADS) { c[0] += x[3 * i]; c[1] += x[3 * i + 1]; c[2] += x[3 * i + 2]; }
  block_sum<float, 3>(c, redf, lane, wave);
  {
    const float cx = c[0] * inv_n, cy = c[1] * inv_n, cz = c[2] * inv_n;
    rotvec_to_matrix(rot[0], rot[1], rot[2], M);
    const float tx = tr[0] + cx, ty = tr[1] + cy, tz = tr[2] + cz;
    for (int i = tid; i < n; i += DDP_DESCENT_THREADS) {
      const float px = x[3 * i] - cx, py = x[3 * i + 1] - cy, pz = x[3 * i + 2] - cz;
      const float ox = M[0] * px + M[1] * py + M[2] * pz + tx, oy = M[3] * px + M[4] * py + M[5] * pz + ty,
                  oz = M[6] * px + M[7] * py + M[8] * pz + tz;
      xt[3 * i] = ox; xt[3 * i + 1] = oy; xt[3 * i + 2] = oz;
      rg[3 * i] = ox; rg[3 * i + 1] = oy; rg[3 * i + 2] = oz;
    }
  }
  __syncthreads();
  if (T == 0) return;                            // (the same for all threads)
  // torsions, in bond order: the atoms of mask_rotate[j] turn about the axis xt[u] - xt[v] through xt[v]
  for (int j = 0; j < T; ++j) {
    const int u = A.bonds[2 * j], v = A.bonds[2 * j + 1];
    if (u < 0 || u >= n || v < 0 || v >= n) continue;   // an entry outside the ligand: no read, no rotation (the same for all threads)
    const float pvx = xt[3 * v], pvy = xt[3 * v + 1], pvz = xt[3 * v + 2];
    const float ax = xt[3 * u] - pvx, ay = xt[3 * u + 1] - pvy, az = xt[3 * u + 2] - pvz;
    const float k = tor[j] / sqrtf(ax * ax + ay * ay + az * az);
    rotvec_to_matrix(ax * k, ay * k, az * k, M);
    __syncthreads();                             // every thread has read the axis before an atom on it may move
    const uint8_t* __restrict__ mk = A.mask_rotate + (size_t)j * n;
    for (int i = tid; i < n; i += DDP_DESCENT_THREADS)
      if (mk[i]) {
        const float px = xt[3 * i] - pvx, py = xt[3 * i + 1] - pvy, pz = xt[3 * i + 2] - pvz;
        xt[3 * i] = M[0] * px + M[1] * py + M[2] * pz + pvx;
        xt[3 * i + 1] = M[3] * px + M[4] * py + M[5] * pz + pvy;
        xt[3 * i + 2] = M[6] * px + M[7] * py + M[8] * pz + pvz;
      }
    __syncthreads();
  }
  // Horn / Kabsch alignment of xt (A) onto rg (B): centroids, covariance S[x][y] = sum (a - ca)_x (b - cb)_y
  float ab[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int i = tid; i < n; i += DDP_DESCENT_THREADS) {
    ab[0] += xt[3 * i]; ab[1] += xt[3 * i + 1]; ab[2] += xt[3 * i + 2];
    ab[3] += rg[3 * i]; ab[4] += rg[3 * i + 1]; ab[5] += rg[3 * i + 2];
  }
  block_sum<float, 6>(ab, redf, lane, wave);
  const float cax = ab[0] * inv_n, cay = ab[1] * inv_n, caz = ab[2] * inv_n, cbx = ab[3] * inv_n, cby = ab[4] * inv_n, cbz = ab[5] * inv_n;
  float S[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int i = tid; i < n; i += DDP_DESCENT_THREADS) {
    const float px = xt[3 * i] - cax, py = xt[3 * i + 1] - cay, pz = xt[3 * i + 2] - caz;
    const float p = rg[3 * i] - cbx, q = rg[3 * i + 1] - cby, r = rg[3 * i + 2] - cbz;
    S[0] += px * p; S[1] += px * q; S[2] += px * r;
    S[3] += py * p; S[4] += py * q; S[5] += py * r;
    S[6] += pz * p; S[7] += pz * q; S[8] += pz * r;
  }
  block_sum<float, 9>(S, redf, lane, wave);
  {
    const float ca[3] = {cax, cay, caz}, cb[3] = {cbx, cby, cbz};
    float R[9], t[3];
    horn_rigid(S, ca, cb, R, t);                 // by every thread, on the same sums: the same bits
    for (int i = tid; i < n; i += DDP_DESCENT_THREADS) {   // (atom i is this thread's alone)
      const float px = xt[3 * i], py = xt[3 * i + 1], pz = xt[3 * i + 2];
      xt[3 * i] = R[0] * px + R[1] * py + R[2] * pz + t[0];
      xt[3 * i + 1] = R[3] * px + R[4] * py + R[5] * pz + t[1];
      xt[3 * i + 2] = R[6] * px + R[7] * py + R[8] * pz + t[2];
    }
  }
  __syncthreads();
}

// ---- the Vinardo-form score of one pose.  A: the kernel's arguments, of which n, m, rec_radii, rec_flags, self_pairs and the constants
// A.form (ddp_score_form_t, handed down to score_pair) are read.  x [n][3], rad [n], lflag [n]: the ligand in LDS, visible to all threads no later than the
// first barrier inside (the caller may stage it right before the call); rs: the sample's receptor in global memory, streamed through
// tile / tflag (LDS, DDP_SCORE_TILE atoms) that all 256 threads fill with coalesced reads.  Wave w owns the ligand atoms w, w + 4, ...;
// its lanes stride over the tile, then over the ligand atoms j with self_pairs[min(i, j)][max(i, j)].  The energy sums stay in
// lane-private accumulators over all the atoms and tiles a lane meets (a fixed sequence) and go through one butterfly at the end;
// with GRAD the gradient of atom i goes through the butterfly once per tile and once for the self pairs, and lane 0 adds it to
// gacc [n][3] (LDS; tiles in increasing order, then the self pairs).  Ends with a barrier, after which we [waves][8] holds every wave's
// partial of the eight unweighted sums (cross, then self: gauss, repulsion, hydrophobic, hbond) and gacc the gradient of inter + intra.
// patch: the tile-load hook, patch(j, r, f) may replace what receptor atom j brings into the tile (coordinates and radius r, flag byte
// f); ScoreTileIdentity, the default, leaves the atom as global memory has it (ddp_pose_score, ddp_pose_minimize), the joint minimiser
// of ddp_minimize_flex.hip puts the moving side-chain atoms in from LDS.
struct ScoreTileIdentity {
  __device__ __forceinline__ void operator()(int, float4&, uint8_t&) const {}
};

template <bool GRAD, class Args, class Patch = ScoreTileIdentity>
__device__ __forceinline__ void score_evaluate(const Args& A, const float* __restrict__ rs, float4* tile, uint8_t* tflag, const float* x,
                                               const float* rad, const uint8_t* lflag, double* gacc, double (*we)[8],
                                               const Patch& patch = Patch()) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = A.n, m = A.m;
  if (GRAD)
    for (int i = tid; i < 3 * n; i += DDP_DESCENT_THREADS) gacc[i] = 0.0;
  const ddp_score_form_t& F = A.form;
  const double cut2 = F.cutoff * F.cutoff;
  ScoreAcc cross = {{0.0, 0.0, 0.0, 0.0}, 0.0, 0.0, 0.0};  // this lane's share, over every atom and tile it meets
  for (int j0 = 0; j0 < m; j0 += DDP_SCORE_TILE) {
    const int mt = min(DDP_SCORE_TILE, m - j0);
    __syncthreads();                             // the previous tile has been used (first pass: the ligand and gacc are visible)
    for (int j = tid; j < mt; j += DDP_DESCENT_THREADS) {
      float4 r = make_float4(rs[3 * (j0 + j)], rs[3 * (j0 + j) + 1], rs[3 * (j0 + j) + 2], A.rec_radii[j0 + j]);
      uint8_t f = A.rec_flags[j0 + j];
      patch(j0 + j, r, f);
      tile[j] = r;
      tflag[j] = f;
    }
    __syncthreads();
    for (int i = wave; i < n; i += DDP_DESCENT_WAVES) {
      const double ri = rad[i];
      if (ri < 0.0) continue;                    // an untyped ligand atom (wave-uniform, no barrier inside)
      const double xi = x[3 * i], yi = x[3 * i + 1], zi = x[3 * i + 2];
      const unsigned fi = lflag[i];
      cross.gx = cross.gy = cross.gz = 0.0;
      for (int j = lane; j < mt; j += 64) {
        const float4 r = tile[j];
        if (r.w < 0.f) continue;                 // an untyped receptor atom
        score_pair<GRAD>(F, cut2, xi - (double)r.x, yi - (double)r.y, zi - (double)r.z, ri + (double)r.w, fi, tflag[j], cross);
      }
      if (GRAD) {
        const double gx = wave_sum(cross.gx), gy = wave_sum(cross.gy), gz = wave_sum(cross.gz);
        if (lane == 0) { gacc[3 * i] += gx; gacc[3 * i + 1] += gy; gacc[3 * i + 2] += gz; }   // (atom i is this wave's alone)
      }
    }
  }
  __syncthreads();                               // m = 0: the ligand and gacc are visible
  ScoreAcc self = {{0.0, 0.0, 0.0, 0.0}, 0.0, 0.0, 0.0};
  for (int i = wave; i < n; i += DDP_DESCENT_WAVES) {
    const double ri = rad[i];
    self.gx = self.gy = self.gz = 0.0;
    if (A.self_pairs && ri >= 0.0) {
      const double xi = x[3 * i], yi = x[3 * i + 1], zi = x[3 * i + 2];
      const unsigned fi = lflag[i];
      for (int j = lane; j < n; j += 64) {
        if (j == i || rad[j] < 0.f || !A.self_pairs[(size_t)min(i, j) * n + max(i, j)]) continue;
        score_pair<GRAD>(F, cut2, xi - (double)x[3 * j], yi - (double)x[3 * j + 1], zi - (double)x[3 * j + 2], ri + (double)rad[j], fi,
                         lflag[j], self);
      }
    }
    if (GRAD) {
      const double gx = wave_sum(self.gx), gy = wave_sum(self.gy), gz = wave_sum(self.gz);
      if (lane == 0) { gacc[3 * i] = gacc[3 * i] + gx; gacc[3 * i + 1] = gacc[3 * i + 1] + gy; gacc[3 * i + 2] = gacc[3 * i + 2] + gz; }
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double c = wave_sum(cross.t[k]), f = wave_sum(self.t[k]);
    if (lane == 0) { we[wave][k] = c; we[wave][4 + k] = f; }
  }
  __syncthreads();
}

// by one thread, after score_evaluate: t[8] = the eight sums over the waves in wave order, inter and intra = the weighted energies
__device__ __forceinline__ void score_totals(const ddp_score_form_t& A, const double (*we)[8], double* t, double& inter, double& intra) {
  for (int k = 0; k < 8; ++k) {
    t[k] = we[0][k];
    for (int w = 1; w < DDP_DESCENT_WAVES; ++w) t[k] += we[w][k];
  }
  inter = A.w_gauss * t[0] + A.w_repulsion * t[1] + A.w_hydrophobic * t[2] + A.w_hbond * t[3];
  // every self pair is met from both ends and counts half each time: exact
  intra = A.w_gauss * (0.5 * t[4]) + A.w_repulsion * (0.5 * t[5]) + A.w_hydrophobic * (0.5 * t[6]) + A.w_hbond * (0.5 * t[7]);
}

// ---- the restraint of the ligand to its anchor `as` (global memory) in a pass of its own, after score_evaluate: wave w sums
// |x_i - as_i|^2 over its atoms w, w + 4, ... in that order (all lanes hold the same value), lane 0 adds the term's gradient to g and
// leaves the wave's sum in wr[wave]; both visible after the caller's next barrier.  A: n and restraint are read.
template <class Args>
__device__ __forceinline__ void descent_ligand_restraint(const Args& A, const float* x, const float* __restrict__ as, double* g, double* wr) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = A.n;
  const double krest = 2.0 * A.restraint / (double)n;
  double er_w = 0.0;
  for (int i = wave; i < n; i += DDP_DESCENT_WAVES) {
    const double xi = x[3 * i], yi = x[3 * i + 1], zi = x[3 * i + 2];
    const double ax = xi - (double)as[3 * i], ay = yi - (double)as[3 * i + 1], az = zi - (double)as[3 * i + 2];
    er_w += ax * ax + ay * ay + az * az;
    if (lane == 0) { g[3 * i] = g[3 * i] + krest * ax; g[3 * i + 1] = g[3 * i + 1] + krest * ay; g[3 * i + 2] = g[3 * i + 2] + krest * az; }
  }
  if (lane == 0) wr[wave] = er_w;
}

// host: the constant checks of ddp_score_form_t, for every entry that takes a form; 0, or DDP_EINVAL with a text that names `who`
static inline int score_check_constants(const ddp_score_form_t* a, const char* who) {
  char msg[128];
  const char* what = nullptr;
  if (!(a->cutoff > 0.0) || !isfinite(a->cutoff)) what = "cutoff must be positive and finite";
  else if (!(a->gauss_width > 0.0) || !(a->hydrophobic_bad > a->hydrophobic_good) || !(a->hbond_bad > a->hbond_good))
    what = "gauss_width must be positive, every ramp must have good < bad";
  if (!what) return 0;
  snprintf(msg, sizeof msg, "%s: %s", who, what);
  return ddp_fail(DDP_EINVAL, msg);
}

#endif
