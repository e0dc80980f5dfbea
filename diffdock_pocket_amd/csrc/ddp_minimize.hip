// ddp_minimize.hip - local minimisation of sampled poses in the Vinardo-form score, the whole backtracking line search of a pose in
// ONE launch (include/ddp_hip.h, ddp_pose_minimize; host side diffdock_pocket_amd/minimize.py, which states the whole definition).
// The launch-by-launch form of the same loop (ddp_pose_score, ddp_refine_direction, ddp_pose_update, ddp_refine_accept) pays four to
// five dependent launches per iteration, and the launches, not the arithmetic, are its cost.  Every pose is independent and one
// workgroup already holds a whole pose, so here one 256-thread workgroup runs all iterations of its pose: the current pose, the trial,
// the rigid copy of the pose map, both gradients, the radii and the flags stay in LDS for the whole call.
// Per iteration: the direction of ddp_refine_direction_kernel (fp64, the same sums in the same order); the pose map of
// ddp_pose_update_kernel in fp32 (rigid move about the centroid, the torsions in bond order, Horn re-alignment through ddp_horn.h:
// every thread runs the 4x4 Jacobi on the same block sums, which costs a SIMD what one thread costs it and saves the barrier that
// publishing the matrix would need); energy and gradient of the trial with the launch plan of ddp_pose_score_kernel (receptor streamed
// through an LDS tile that all threads fill with coalesced reads, wave w owns the ligand atoms w, w + 4, ..., butterflies); the accept
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
#include "ddp_score_pair.h"

#define DDP_MZ_THREADS 256
#define DDP_MZ_WAVES (DDP_MZ_THREADS / 64)
#define DDP_MZ_TILE 1024
// fixed part of the LDS plan, every carve a multiple of 16 bytes: the receptor tile and its flag bytes, then the reduction scratch
#define DDP_MZ_WE_BYTES (DDP_MZ_WAVES * 10 * 8)      // [waves][10] fp64: the energy partials of the evaluation
#define DDP_MZ_RED_BYTES (DDP_MZ_WAVES * 16 * 8)     // [waves][16] fp64 (or fp32): block sums of the direction and the pose map
#define DDP_MZ_FIXED_BYTES (DDP_MZ_TILE * 16 + DDP_MZ_TILE + DDP_MZ_WE_BYTES + DDP_MZ_RED_BYTES + 64)

static_assert(DDP_MINIMIZE_MAX_TORSIONS * sizeof(float) <= DDP_MZ_TILE * sizeof(float4), "the torsion steps live in the tile between two evaluations");
static_assert(DDP_MZ_FIXED_BYTES % 16 == 0, "dynamic LDS carves stay 16-byte aligned");
static_assert(DDP_MZ_FIXED_BYTES + 89 * DDP_MINIMIZE_MAX_ATOMS <= 64 * 1024, "the LDS plan fits the 64 KiB a plain launch may ask for");

struct MzLds {
  float4* tile;        // [DDP_MZ_TILE] receptor x, y, z, radius; between two evaluations its first floats hold the torsion steps
  uint8_t* tflag;      // [DDP_MZ_TILE]
  double (*we)[10];    // [waves][10]
  double (*red)[16];   // [waves][16]
  double* et;          // [4] the energies of the last evaluation
  double* g;           // [2][n][3] gradients: of the current pose and of the trial (which is which changes with every accept)
  float* x;            // [2][n][3] the current pose and the trial
  float* rg;           // [n][3] the rigid copy of the pose map
  float* rad;          // [n]
  uint8_t* lflag;      // [n]
};

// block sum of K values, all threads get the result: butterfly, then the waves in wave order (the sums of
// ddp_refine_direction_kernel).  Two barriers: the first frees `red` of the previous sum's readers, the second publishes this one.
template <typename T, int K>
__device__ __forceinline__ void mz_block_sum(T* v, T (*red)[16 * sizeof(double) / sizeof(T)], int lane, int wave) {
#pragma unroll
  for (int k = 0; k < K; ++k) {
    T a = v[k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) a += __shfl_xor(a, off);
    v[k] = a;
  }
  __syncthreads();
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) red[wave][k] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) {
    T acc = red[0][k];
    for (int w = 1; w < DDP_MZ_WAVES; ++w) acc += red[w][k];
    v[k] = acc;
  }
}

__device__ __forceinline__ void mz_rotvec_to_matrix(float vx, float vy, float vz, float* R) {
  // Rodrigues; small-angle series below 1e-6 (as ddp_pose.hip)
  const float ang = sqrtf(vx * vx + vy * vy + vz * vz);
  float a, b;
  if (ang < 1e-6f) {
    a = 1.0f - ang * ang / 6.0f;
    b = 0.5f - ang * ang / 24.0f;
  } else {
    a = sinf(ang) / ang;
    b = (1.0f - cosf(ang)) / (ang * ang);
  }
  const float xx = vx * vx, yy = vy * vy, zz = vz * vz, xy = vx * vy, xz = vx * vz, yz = vy * vz;
  R[0] = 1.f - b * (yy + zz); R[1] = -a * vz + b * xy;     R[2] = a * vy + b * xz;
  R[3] = a * vz + b * xy;     R[4] = 1.f - b * (xx + zz);  R[5] = -a * vx + b * yz;
  R[6] = -a * vy + b * xz;    R[7] = a * vx + b * yz;      R[8] = 1.f - b * (xx + yy);
}

// Energy [inter, intra, restraint term, E] -> L.et and gradient -> g of the pose x (LDS, visible to all threads on entry).  Ends with
// a barrier: L.et and g are visible on return.  The sums are those of ddp_pose_score_kernel plus the restraint of
// ddp_refine_energy_kernel.
__device__ __forceinline__ void mz_evaluate(const ddp_minimize_args_t& A, const MzLds& L, const float* __restrict__ rs,
                                         const float* __restrict__ as, const float* x, double* g) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = A.n, m = A.m;
  const float* rad = L.rad;
  const uint8_t* lflag = L.lflag;
  for (int i = tid; i < 3 * n; i += DDP_MZ_THREADS) g[i] = 0.0;
  const double cut2 = A.cutoff * A.cutoff;
  const double krest = 2.0 * A.restraint / (double)n;
  ScoreAcc cross = {{0.0, 0.0, 0.0, 0.0}, 0.0, 0.0, 0.0};
  for (int j0 = 0; j0 < m; j0 += DDP_MZ_TILE) {
    const int mt = min(DDP_MZ_TILE, m - j0);
    __syncthreads();                             // the tile is free (first pass: g is zero for everybody)
    for (int j = tid; j < mt; j += DDP_MZ_THREADS) {
      L.tile[j] = make_float4(rs[3 * (j0 + j)], rs[3 * (j0 + j) + 1], rs[3 * (j0 + j) + 2], A.rec_radii[j0 + j]);
      L.tflag[j] = A.rec_flags[j0 + j];
    }
    __syncthreads();
    for (int i = wave; i < n; i += DDP_MZ_WAVES) {
      const double ri = rad[i];
      if (ri < 0.0) continue;                    // an untyped ligand atom (wave-uniform, no barrier inside)
      const double xi = x[3 * i], yi = x[3 * i + 1], zi = x[3 * i + 2];
      const unsigned fi = lflag[i];
      cross.gx = cross.gy = cross.gz = 0.0;
      for (int j = lane; j < mt; j += 64) {
        const float4 r = L.tile[j];
        if (r.w < 0.f) continue;                 // an untyped receptor atom
        score_pair<true>(A, cut2, xi - (double)r.x, yi - (double)r.y, zi - (double)r.z, ri + (double)r.w, fi, L.tflag[j], cross);
      }
      const double gx = score_wave_sum(cross.gx), gy = score_wave_sum(cross.gy), gz = score_wave_sum(cross.gz);
      if (lane == 0) { g[3 * i] += gx; g[3 * i + 1] += gy; g[3 * i + 2] += gz; }   // (atom i is this wave's alone)
    }
  }
  __syncthreads();                               // m = 0: g is zero for everybody
  ScoreAcc self = {{0.0, 0.0, 0.0, 0.0}, 0.0, 0.0, 0.0};
  double er_w = 0.0;                             // the restraint sum of this wave's atoms (all lanes hold the same value)
  for (int i = wave; i < n; i += DDP_MZ_WAVES) {
    const double ri = rad[i];
    const double xi = x[3 * i], yi = x[3 * i + 1], zi = x[3 * i + 2];
    self.gx = self.gy = self.gz = 0.0;
    if (A.self_pairs && ri >= 0.0) {
      const unsigned fi = lflag[i];
      for (int j = lane; j < n; j += 64) {
        if (j == i || rad[j] < 0.f || !A.self_pairs[(size_t)min(i, j) * n + max(i, j)]) continue;
        score_pair<true>(A, cut2, xi - (double)x[3 * j], yi - (double)x[3 * j + 1], zi - (double)x[3 * j + 2], ri + (double)rad[j], fi,
                         lflag[j], self);
      }
    }
    const double gx = score_wave_sum(self.gx), gy = score_wave_sum(self.gy), gz = score_wave_sum(self.gz);
    const double ax = xi - (double)as[3 * i], ay = yi - (double)as[3 * i + 1], az = zi - (double)as[3 * i + 2];
    er_w += ax * ax + ay * ay + az * az;
    if (lane == 0) {
      g[3 * i] = (g[3 * i] + gx) + krest * ax; g[3 * i + 1] = (g[3 * i + 1] + gy) + krest * ay; g[3 * i + 2] = (g[3 * i + 2] + gz) + krest * az;
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double c = score_wave_sum(cross.t[k]), f = score_wave_sum(self.t[k]);
    if (lane == 0) { L.we[wave][k] = c; L.we[wave][4 + k] = f; }
  }
  if (lane == 0) L.we[wave][8] = er_w;
  __syncthreads();
  if (tid == 0) {
    double t[9];
    for (int k = 0; k < 9; ++k) {
      t[k] = L.we[0][k];
      for (int w = 1; w < DDP_MZ_WAVES; ++w) t[k] += L.we[w][k];
    }
    const double inter = A.w_gauss * t[0] + A.w_repulsion * t[1] + A.w_hydrophobic * t[2] + A.w_hbond * t[3];
    // every self pair is met from both ends and counts half each time: exact
    const double intra = A.w_gauss * (0.5 * t[4]) + A.w_repulsion * (0.5 * t[5]) + A.w_hydrophobic * (0.5 * t[6]) + A.w_hbond * (0.5 * t[7]);
    const double rest = A.restraint * (t[8] / (double)n);
    L.et[0] = inter; L.et[1] = intra; L.et[2] = rest; L.et[3] = (inter + intra) + rest;
  }
  __syncthreads();
}

// tr, rot (registers of every thread) and tor (LDS, L.tile's first n_tor floats) = step * the inertia-scaled descent direction of g
// at x, rounded to fp32: the arithmetic of ddp_refine_direction_kernel.  Ends with a barrier: tor is visible on return.
__device__ __forceinline__ void mz_direction(const ddp_minimize_args_t& A, const MzLds& L, const float* x, const double* g, double step,
                                             float* tr, float* rot) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = A.n, T = A.n_tor;
  float* tor = (float*)L.tile;
  double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int i = tid; i < n; i += DDP_MZ_THREADS) {
    v[0] += (double)x[3 * i]; v[1] += (double)x[3 * i + 1]; v[2] += (double)x[3 * i + 2];
    v[3] += g[3 * i]; v[4] += g[3 * i + 1]; v[5] += g[3 * i + 2];
  }
  mz_block_sum<double, 6>(v, L.red, lane, wave);
  const double cx = v[0] / n, cy = v[1] / n, cz = v[2] / n;
  tr[0] = (float)(step * (-v[3] / n)); tr[1] = (float)(step * (-v[4] / n)); tr[2] = (float)(step * (-v[5] / n));
  double r[4] = {0.0, 0.0, 0.0, 0.0};
  for (int i = tid; i < n; i += DDP_MZ_THREADS) {
    const double px = (double)x[3 * i] - cx, py = (double)x[3 * i + 1] - cy, pz = (double)x[3 * i + 2] - cz;
    const double gx = g[3 * i], gy = g[3 * i + 1], gz = g[3 * i + 2];
    r[0] += py * gz - pz * gy; r[1] += pz * gx - px * gz; r[2] += px * gy - py * gx;
    r[3] += px * px + py * py + pz * pz;
  }
  mz_block_sum<double, 4>(r, L.red, lane, wave);
  for (int k = 0; k < 3; ++k) rot[k] = (float)(step * (r[3] == 0.0 ? 0.0 : -r[k] / r[3]));
  for (int b = wave; b < T; b += DDP_MZ_WAVES) {
    const int u = A.bonds[2 * b], w = A.bonds[2 * b + 1];
    double num = 0.0, den = 0.0;
    if (u >= 0 && u < n && w >= 0 && w < n) {    // an entry outside the ligand: no read, the bond gets 0
      const double vx = x[3 * w], vy = x[3 * w + 1], vz = x[3 * w + 2];
      double ux = (double)x[3 * u] - vx, uy = (double)x[3 * u + 1] - vy, uz = (double)x[3 * u + 2] - vz;
      const double len = sqrt(ux * ux + uy * uy + uz * uz);
      ux /= len; uy /= len; uz /= len;
      const uint8_t* __restrict__ mk = A.mask_rotate + (size_t)b * n;
      for (int i = lane; i < n; i += 64) {
        if (!mk[i] || i == u || i == w) continue;  // the bond's own atoms lie on the axis: no lever, exactly
        const double px = (double)x[3 * i] - vx, py = (double)x[3 * i + 1] - vy, pz = (double)x[3 * i + 2] - vz;
        const double ax = uy * pz - uz * py, ay = uz * px - ux * pz, az = ux * py - uy * px;
        num += g[3 * i] * ax + g[3 * i + 1] * ay + g[3 * i + 2] * az;
        den += ax * ax + ay * ay + az * az;
      }
    }
    num = score_wave_sum(num); den = score_wave_sum(den);
    if (lane == 0) tor[b] = (float)(step * (den == 0.0 ? 0.0 : -num / den));
  }
  __syncthreads();
}

// xt = the pose map of ddp_pose_update_kernel applied to x with (tr, rot, tor), fp32.  Ends with a barrier: xt is visible on return.
__device__ __forceinline__ void mz_pose_update(const ddp_minimize_args_t& A, const MzLds& L, const float* x, float* xt, const float* tr,
                                               const float* rot) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = A.n, T = A.n_tor;
  float(*redf)[32] = (float(*)[32])L.red;
  const float* tor = (const float*)L.tile;
  float* rg = L.rg;
  const float inv_n = 1.0f / (float)n;
  float M[9];
  // rigid move about the centre: (x - c) R^T + tr + c
  float c[3] = {0.f, 0.f, 0.f};
  for (int i = tid; i < n; i += DDP_MZ_THREADS) { c[0] += x[3 * i]; c[1] += x[3 * i + 1]; c[2] += x[3 * i + 2]; }
  mz_block_sum<float, 3>(c, redf, lane, wave);
  {
    const float cx = c[0] * inv_n, cy = c[1] * inv_n, cz = c[2] * inv_n;
    mz_rotvec_to_matrix(rot[0], rot[1], rot[2], M);
    const float tx = tr[0] + cx, ty = tr[1] + cy, tz = tr[2] + cz;
    for (int i = tid; i < n; i += DDP_MZ_THREADS) {
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
    mz_rotvec_to_matrix(ax * k, ay * k, az * k, M);
    __syncthreads();                             // every thread has read the axis before an atom on it may move
    const uint8_t* __restrict__ mk = A.mask_rotate + (size_t)j * n;
    for (int i = tid; i < n; i += DDP_MZ_THREADS)
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
  for (int i = tid; i < n; i += DDP_MZ_THREADS) {
    ab[0] += xt[3 * i]; ab[1] += xt[3 * i + 1]; ab[2] += xt[3 * i + 2];
    ab[3] += rg[3 * i]; ab[4] += rg[3 * i + 1]; ab[5] += rg[3 * i + 2];
  }
  mz_block_sum<float, 6>(ab, redf, lane, wave);
  const float cax = ab[0] * inv_n, cay = ab[1] * inv_n, caz = ab[2] * inv_n, cbx = ab[3] * inv_n, cby = ab[4] * inv_n, cbz = ab[5] * inv_n;
  float S[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int i = tid; i < n; i += DDP_MZ_THREADS) {
    const float px = xt[3 * i] - cax, py = xt[3 * i + 1] - cay, pz = xt[3 * i + 2] - caz;
    const float p = rg[3 * i] - cbx, q = rg[3 * i + 1] - cby, r = rg[3 * i + 2] - cbz;
    S[0] += px * p; S[1] += px * q; S[2] += px * r;
    S[3] += py * p; S[4] += py * q; S[5] += py * r;
    S[6] += pz * p; S[7] += pz * q; S[8] += pz * r;
  }
  mz_block_sum<float, 9>(S, redf, lane, wave);
  {
    const double S3[3][3] = {{S[0], S[1], S[2]}, {S[3], S[4], S[5]}, {S[6], S[7], S[8]}};
    double q[4];
    horn_quaternion(S3, q);                      // by every thread, on the same sums: the same bits
    const double w = q[0], qx = q[1], qy = q[2], qz = q[3];
    const float R[9] = {(float)(1 - 2 * (qy * qy + qz * qz)), (float)(2 * (qx * qy - qz * w)), (float)(2 * (qx * qz + qy * w)),
                        (float)(2 * (qx * qy + qz * w)), (float)(1 - 2 * (qx * qx + qz * qz)), (float)(2 * (qy * qz - qx * w)),
                        (float)(2 * (qx * qz - qy * w)), (float)(2 * (qy * qz + qx * w)), (float)(1 - 2 * (qx * qx + qy * qy))};
    // t = cb - R ca
    const float t0 = cbx - (R[0] * cax + R[1] * cay + R[2] * caz), t1 = cby - (R[3] * cax + R[4] * cay + R[5] * caz),
                t2 = cbz - (R[6] * cax + R[7] * cay + R[8] * caz);
    for (int i = tid; i < n; i += DDP_MZ_THREADS) {   // (atom i is this thread's alone)
      const float px = xt[3 * i], py = xt[3 * i + 1], pz = xt[3 * i + 2];
      xt[3 * i] = R[0] * px + R[1] * py + R[2] * pz + t0;
      xt[3 * i + 1] = R[3] * px + R[4] * py + R[5] * pz + t1;
      xt[3 * i + 2] = R[6] * px + R[7] * py + R[8] * pz + t2;
    }
  }
  __syncthreads();
}

__global__ __launch_bounds__(DDP_MZ_THREADS) void ddp_pose_minimize_kernel(const ddp_minimize_args_t A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char mz_lds[];
  const int s = blockIdx.x, tid = threadIdx.x, n = A.n, S = A.n_samples;
  MzLds L;
  unsigned char* p = mz_lds;
  L.tile = (float4*)p; p += DDP_MZ_TILE * sizeof(float4);
  L.tflag = p; p += DDP_MZ_TILE;
  L.we = (double(*)[10])p; p += DDP_MZ_WE_BYTES;
  L.red = (double(*)[16])p; p += DDP_MZ_RED_BYTES;
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
      float tr[3], rot[3];
      mz_direction(A, L, L.x + cur * 3 * n, L.g + cur * 3 * n, step, tr, rot);
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
  if (a->n_samples < 0 || a->n <= 0 || a->m < 0 || a->n_tor < 0 || (a->rec_stride != 0 && a->rec_stride < 3 * a->m))
    return ddp_fail(DDP_EINVAL, "ddp_pose_minimize: shape");
  if (a->n > DDP_MINIMIZE_MAX_ATOMS) return ddp_fail(DDP_ELIMIT, "ddp_pose_minimize: more than DDP_MINIMIZE_MAX_ATOMS ligand atoms");
  if (a->n_tor > DDP_MINIMIZE_MAX_TORSIONS) return ddp_fail(DDP_ELIMIT, "ddp_pose_minimize: more than DDP_MINIMIZE_MAX_TORSIONS rotatable bonds");
  if (!a->pos || !a->anchor || !a->lig_radii || !a->lig_flags || !a->step || !a->accepted || !a->energy_in || !a->energy_out ||
      (a->m > 0 && (!a->rec || !a->rec_radii || !a->rec_flags)) || (a->n_tor > 0 && (!a->bonds || !a->mask_rotate)))
    return ddp_fail(DDP_EINVAL, "ddp_pose_minimize: null argument");
  if (a->iterations < 0 || !(a->restraint >= 0.0)) return ddp_fail(DDP_EINVAL, "ddp_pose_minimize: iterations or restraint < 0");
  if (!(a->cutoff > 0.0) || !isfinite(a->cutoff)) return ddp_fail(DDP_EINVAL, "ddp_pose_minimize: cutoff must be positive and finite");
  if (!(a->gauss_width > 0.0) || !(a->hydrophobic_bad > a->hydrophobic_good) || !(a->hbond_bad > a->hbond_good))
    return ddp_fail(DDP_EINVAL, "ddp_pose_minimize: gauss_width must be positive, every ramp must have good < bad");
  // the fixed part (receptor tile, its flags, reduction scratch) + two gradients, three coordinate sets, radii and flags per atom:
  // 17.9 KiB + 89 n, 62.4 KiB at the atom limit
  const size_t lds = DDP_MZ_FIXED_BYTES + (size_t)89 * a->n;
  hipLaunchKernelGGL(ddp_pose_minimize_kernel, dim3(a->n_samples), dim3(DDP_MZ_THREADS), lds, (hipStream_t)stream, *a);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return ddp_fail_hip(err, "ddp_pose_minimize launch");
  return 0;
}
