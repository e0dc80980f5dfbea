// ddp_profile.hip - the per-residue interaction profile of sampled poses (include/ddp_hip.h, ddp_pose_profile; host side
// diffdock_pocket_amd/interactions.py, which states the whole definition).  The pair arithmetic is score_pair of ddp_score_pair.h, the
// one ddp_pose_score sums over the whole receptor; here it is summed per residue, with the pair count and the closest approach.
// The launch plan is the family's (ddp_score.hip): one 256-thread workgroup per sample, the ligand staged in LDS.  Wave w owns the
// residues w, w + 4, ...; it takes a residue's atoms 64 at a time, one per lane (radius, flags, the distance to the ligand's bounding
// sphere, the finiteness of the coordinates), and then walks the atoms that can have a pair: the atom is broadcast from its lane and
// the 64 lanes stride over the ligand atoms (the first 64 of which sit in registers).  Residues are short (a dozen heavy atoms) and
// ligands are not, so this keeps more lanes busy than a split of the residue's atoms over the lanes.  Every sum is lane-private over
// a fixed sequence of pairs and goes through one butterfly per residue (none where no lane met a pair: the result is the no-pair
// result either way); lane 0 writes.  No atomics: two launches give the same bits, and a sample's result does not depend on the
// other samples of the launch.  All arithmetic is fp64 on the fp32 inputs (converted first).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ddp_hip.h"
#include "ddp_internal.h"
#include "ddp_pose_descent.h"

// wave minimum, all lanes get it (fmin of two equal-rank partial minima per stage: the same bits in every lane)
__device__ __forceinline__ double profile_wave_min(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmin(v, __shfl_xor(v, off));
  return v;
}

// the value lane `src` holds, src wave-uniform
__device__ __forceinline__ float profile_lane(float v, int src) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src)); }

__device__ __forceinline__ bool profile_finite3(float a, float b, float c) { return isfinite(a) && isfinite(b) && isfinite(c); }

// LDS: the sample's ligand coordinates, radii and flag bytes (fp32 as they come): 17 n bytes, 17 KiB at the atom limit.
__global__ __launch_bounds__(DDP_DESCENT_THREADS) void ddp_pose_profile_kernel(const ddp_profile_args_t A) {
  extern __shared__ float lds[];
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = A.n, m = A.m, R = A.n_res;
  float* x = lds;                                         // [n][3]
  float* rad = x + 3 * n;                                 // [n]
  uint8_t* lflag = (uint8_t*)(rad + n);                   // [n]
  __shared__ double red[DDP_DESCENT_WAVES * 5];
  const float* __restrict__ ls = A.pos + (size_t)s * n * 3;
  for (int i = tid; i < 3 * n; i += DDP_DESCENT_THREADS) x[i] = ls[i];
  for (int i = tid; i < n; i += DDP_DESCENT_THREADS) { rad[i] = A.lig_radii[i]; lflag[i] = A.lig_flags[i]; }
  __syncthreads();
  // the typed ligand atoms: how many, how many of them with a non-finite coordinate, their centre and the radius of the sphere about
  // it that holds them.  Any point serves as the centre: the test below is the triangle inequality.
  double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int i = tid; i < n; i += DDP_DESCENT_THREADS) {
    if (rad[i] < 0.f) continue;
    v[0] += 1.0;
    if (!profile_finite3(x[3 * i], x[3 * i + 1], x[3 * i + 2])) { v[1] += 1.0; continue; }
    v[2] += (double)x[3 * i]; v[3] += (double)x[3 * i + 1]; v[4] += (double)x[3 * i + 2];
  }
  block_sum<double, 5>(v, red, lane, wave);
  const bool lig_any = v[0] > 0.0, lig_bad = v[1] > 0.0;
  const double cx = lig_any ? v[2] / v[0] : 0.0, cy = lig_any ? v[3] / v[0] : 0.0, cz = lig_any ? v[4] / v[0] : 0.0;
  double rho2 = 0.0;
  for (int i = tid; i < n; i += DDP_DESCENT_THREADS) {
    if (rad[i] < 0.f) continue;
    const double px = (double)x[3 * i] - cx, py = (double)x[3 * i + 1] - cy, pz = (double)x[3 * i + 2] - cz;
    rho2 = fmax(rho2, px * px + py * py + pz * pz);
  }
  rho2 = -profile_wave_min(-rho2);
  __syncthreads();                                       // `red` is free of the sum's readers
  if (lane == 0) red[wave] = rho2;
  __syncthreads();
  for (int w = 0; w < DDP_DESCENT_WAVES; ++w) rho2 = fmax(rho2, red[w]);
  // a receptor atom at more than `reach` from the centre has every ligand atom at cutoff or more: |r - x_i| >= |r - c| - |x_i - c|.
  // The factor covers the rounding of the three distances (a few 2^-53 each) with room to spare, so the pairs passed over are
  // exactly pairs that score_pair would have rejected.
  const ddp_score_form_t& F = A.form;
  const double reach = (F.cutoff + sqrt(rho2)) * (1.0 + 0x1p-40), reach2 = reach * reach;
  const double cut2 = F.cutoff * F.cutoff;
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  const float* __restrict__ rs = A.rec + (size_t)s * A.rec_stride;
  double* __restrict__ prof = A.profile + (size_t)s * R * 7;
  uint8_t* __restrict__ bits = A.bits + (size_t)s * R;

  // A ligand of up to 64 atoms has one atom per lane: that atom stays in registers for all the residues (the others come from LDS).
  const bool has0 = lane < n && rad[lane] >= 0.f;
  const double x0 = has0 ? (double)x[3 * lane] : 0.0, y0 = has0 ? (double)x[3 * lane + 1] : 0.0, z0 = has0 ? (double)x[3 * lane + 2] : 0.0;
  const double r0 = has0 ? (double)rad[lane] : 0.0;
  const unsigned f0 = has0 ? lflag[lane] : 0u;
  // One residue atom per lane: radius, coordinates and flag byte of atom c0 + lane (lanes past the residue's end: untyped).
  struct Chunk { float x, y, z, r; unsigned f; };
  auto load_chunk = [&](int c0, int c1) {
    Chunk c = {0.f, 0.f, 0.f, -1.f, 0u};
    const int j = c0 + lane;
    if (j < c1) { c.r = A.rec_radii[j]; c.x = rs[3 * j]; c.y = rs[3 * j + 1]; c.z = rs[3 * j + 2]; c.f = A.rec_flags[j]; }
    return c;
  };
  for (int r = wave; r < R; r += DDP_DESCENT_WAVES) {    // (wave-uniform: no barrier inside)
    const int j0 = min(max(A.res_ptr[r], 0), m), j1 = min(max(A.res_ptr[r + 1], 0), m);
    ScoreAcc acc = {{0.0, 0.0, 0.0, 0.0}, 0.0, 0.0, 0.0};
    int count = 0;
    double dmin2 = INFINITY;
    bool res_bad = false, any_near = false;
    auto pair = [&](double dx, double dy, double dz, double rsum, unsigned fi, unsigned fj) {
      const double d2 = dx * dx + dy * dy + dz * dz;
      if (d2 < cut2) { count += 1; dmin2 = fmin(dmin2, d2); }
      score_pair<false>(F, cut2, dx, dy, dz, rsum, fi, fj, acc);
    };
    for (int c0 = j0; c0 < j1 && !lig_bad; c0 += 64) {
      const Chunk cur = load_chunk(c0, j1);
      const float rx = cur.x, ry = cur.y, rz = cur.z, rr = cur.r;
      const unsigned rf = cur.f;
      bool bad = false, near = false;
      if (rr >= 0.f) {
        bad = !profile_finite3(rx, ry, rz);
        const double px = (double)rx - cx, py = (double)ry - cy, pz = (double)rz - cz;
        near = lig_any && !bad && !(px * px + py * py + pz * pz > reach2);
      }
      res_bad = res_bad || __ballot(bad) != 0ull;
      unsigned long long todo = __ballot(near);
      any_near = any_near || todo != 0ull;
      while (todo) {                                     // the atoms of this chunk that can have a pair, in atom order
        const int src = __ffsll(todo) - 1;               // (wave-uniform: the atom comes over by v_readlane)
        todo &= todo - 1ull;
        const double xj = profile_lane(rx, src), yj = profile_lane(ry, src), zj = profile_lane(rz, src), rj = profile_lane(rr, src);
        const unsigned fj = (unsigned)__builtin_amdgcn_readlane((int)rf, src);
        if (has0) pair(x0 - xj, y0 - yj, z0 - zj, r0 + rj, f0, fj);
        for (int i = lane + 64; i < n; i += 64) {
          const double ri = rad[i];
          if (ri < 0.0) continue;                        // an untyped ligand atom
          pair((double)x[3 * i] - xj, (double)x[3 * i + 1] - yj, (double)x[3 * i + 2] - zj, ri + rj, lflag[i], fj);
        }
      }
    }
    double t[4] = {0.0, 0.0, 0.0, 0.0};
    // (wave-uniform) no atom within reach, or none of the walked atoms with a pair: every lane holds the no-pair result, which is
    // written as it is, without the butterfly
    if (any_near && __ballot(count > 0) != 0ull) {
#pragma unroll
      for (int k = 0; k < 4; ++k) t[k] = wave_sum(acc.t[k]);
      count = wave_sum(count);
      dmin2 = profile_wave_min(dmin2);
    }
    if (lane == 0) {
      double* p = prof + (size_t)r * 7;
      if (lig_bad || res_bad) {
        p[0] = nan; p[1] = nan; p[2] = nan; p[3] = nan; p[4] = nan; p[5] = nan; p[6] = 0.0;
        bits[r] = 0;
      } else {
        const double dmin = sqrt(dmin2);
        p[0] = t[0]; p[1] = t[1]; p[2] = t[2]; p[3] = t[3];
        p[4] = F.w_gauss * t[0] + F.w_repulsion * t[1] + F.w_hydrophobic * t[2] + F.w_hbond * t[3];
        p[5] = dmin;
        p[6] = (double)count;
        bits[r] = (uint8_t)((dmin < A.contact_distance ? 1 : 0) | (t[2] > 0.0 ? 2 : 0) | (t[3] > 0.0 ? 4 : 0));
      }
    }
  }
}

extern "C" int ddp_pose_profile(const ddp_profile_args_t* a, void* stream) {
  if (!a) return ddp_fail(DDP_EINVAL, "ddp_pose_profile: null argument struct");
  if (a->n_samples == 0 || a->n_res == 0) return 0;
  if (const int rc = ddp_pose_check_shape("ddp_pose_profile", a->n_samples, a->n, a->m, a->rec_stride, a->n_res >= 0)) return rc;
  if (const int rc = DDP_POSE_CHECK_ATOMS("ddp_pose_profile", a->n, DDP_EVAL_MAX_ATOMS)) return rc;
  if (!a->pos || !a->lig_radii || !a->lig_flags || !a->res_ptr || !a->profile || !a->bits ||
      (a->m > 0 && (!a->rec || !a->rec_radii || !a->rec_flags)))
    return ddp_fail(DDP_EINVAL, "ddp_pose_profile: null argument");
  if (const int rc = score_check_constants(&a->form, "ddp_pose_profile")) return rc;
  if (!(a->contact_distance > 0.0) || !isfinite(a->contact_distance))
    return ddp_fail(DDP_EINVAL, "ddp_pose_profile: contact_distance must be positive and finite");
  const size_t lds = (size_t)a->n * (4 * sizeof(float) + 1);
  hipLaunchKernelGGL(ddp_pose_profile_kernel, dim3(a->n_samples), dim3(DDP_DESCENT_THREADS), lds, (hipStream_t)stream, *a);
  return ddp_launch_result("ddp_pose_profile");
}
