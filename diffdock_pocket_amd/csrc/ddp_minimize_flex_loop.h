// ddp_minimize_flex_loop.h - the joint line search of ligand and flexible side chains as a device function: the LDS plan, the
// evaluation of E, the side-chain direction and map, and the iteration loop with its single call site of the evaluation - the
// counterpart of ddp_minimize_loop.h with a second molecule in the state.  ddp_pose_minimize_flex_kernel (ddp_minimize_flex.hip) runs
// it once per pose, ddp_pose_search_flex_kernel (ddp_search_flex.hip) once per cycle of a replica.  Both are one 256-thread workgroup
// per row; diffdock_pocket_amd/minimize_flex.py states the algorithm.  The workgroup holds, for the whole call, what ddp_pose_minimize
// holds for the ligand and, for the n_mov moving receptor atoms, the current and the trial coordinates, both gradients, radii, flags,
// their receptor indices and the side-chain steps.  The energy of a state is a function of its fp32 coordinates, the receptor's
// static atoms and the anchors only, whichever kernel, iteration or launch evaluates it.
// One evaluation:
//   1. score_evaluate of ddp_pose_descent.h for the ligand side.  Its tile-load hook (FxPatch) puts the moving atoms in from LDS as the
//      receptor tile is loaded: a binary search of the atom's index in the sorted `mov` (at most 9 probes of LDS per loaded atom) is the
//      slot lookup, so the trial receptor never goes through global memory.  The hook also marks a moving atom in bit 7 of its flag
//      byte, which the pair arithmetic does not read.
//   2. the ligand restraint of ddp_pose_minimize (descent_ligand_restraint of ddp_pose_descent.h).
//   3. the second pass: wave w owns the moving atoms w, w + 4, ...  Its lanes stride over the ligand atoms in LDS (the receptor-side
//      gradient of inter, by gather), then over the receptor tile for the partners of sc_pairs (the energy and gradient of sc; a
//      partner that moves itself counts half in the energy, it is met again from its own row), then lane 0 adds the side-chain
//      restraint.  m <= one tile: the tile that step 1 loaded is still there and is used as it is.
// Every sum has a fixed order (ddp_pose_descent.h): butterflies inside a wave, the waves in wave order, the tiles in increasing order.
// No atomics.  No data-dependent control flow around a barrier: trip counts and the conditions that skip a barrier (an index outside
// the receptor, m <= one tile) are kernel arguments or table entries, the same for all 256 threads.
#ifndef DDP_MINIMIZE_FLEX_LOOP_H
#define DDP_MINIMIZE_FLEX_LOOP_H
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ddp_hip.h"
#include "ddp_internal.h"
#include "ddp_horn.h"
#include "ddp_pose_descent.h"

#define DDP_FX_THREADS DDP_DESCENT_THREADS
#define DDP_FX_WAVES DDP_DESCENT_WAVES
#define DDP_FX_TILE DDP_SCORE_TILE
#define DDP_FX_MOVING 0x80u                          // flag bit of a tile entry that the hook put in
// fixed part of the LDS plan, every carve a multiple of 16 bytes: that of ddp_minimize.hip, then the second pass's partial sums
#define DDP_FX_WE_BYTES (DDP_FX_WAVES * 10 * 8)      // [waves][8] fp64 of score_evaluate, then [waves] of the ligand restraint
#define DDP_FX_RED_BYTES (DDP_FX_WAVES * 16 * 8)     // block sums of the direction and the pose map
#define DDP_FX_WE2_BYTES 192                         // [waves][4] fp64 of sc, then [waves] of the side-chain restraint
#define DDP_FX_FIXED_BYTES (DDP_FX_TILE * 16 + DDP_FX_TILE + DDP_FX_WE_BYTES + DDP_FX_RED_BYTES + 64 + DDP_FX_WE2_BYTES)

static_assert(DDP_MINIMIZE_MAX_TORSIONS * sizeof(float) <= DDP_FX_TILE * sizeof(float4), "the torsion steps live in the tile between two evaluations");
static_assert(DDP_FX_FIXED_BYTES % 16 == 0, "dynamic LDS carves stay 16-byte aligned");
static_assert(DDP_FX_FIXED_BYTES == 18496, "the header states the fixed part of the plan");
static_assert(DDP_FX_FIXED_BYTES + DDP_MINIMIZE_FLEX_MAX_STATE_BYTES <= 64 * 1024, "the LDS plan fits the 64 KiB a plain launch may ask for");
static_assert(DDP_FX_WAVES * 5 * 8 <= DDP_FX_WE2_BYTES, "the second pass's partial sums");

struct FxLds {
  float4* tile;        // [DDP_FX_TILE] receptor x, y, z, radius; between two evaluations its first floats hold the ligand torsion steps
  uint8_t* tflag;      // [DDP_FX_TILE]
  double (*we)[8];     // [waves][8]
  double* wr;          // [waves] the ligand restraint sums of the waves
  double* red;         // scratch of block_sum
  double* et;          // [6] the energies of the last evaluation
  double (*we2)[4];    // [waves][4] the sc sums of the waves
  double* wr2;         // [waves] the side-chain restraint sums of the waves
  double* g;           // [2][n][3] ligand gradients: of the current pose and of the trial
  double* gm;          // [2][n_mov][3] the same of the moving atoms
  float* x;            // [2][n][3] the current pose and the trial
  float* ym;           // [2][n_mov][3] the same of the moving atoms
  float* rg;           // [n][3] the rigid copy of the pose map
  float* rad;          // [n]
  float* mrad;         // [n_mov] radius; negative: untyped, or an index outside the receptor - the atom takes part in nothing
  int32_t* mov;        // [n_mov]
  float* scstep;       // [n_sc] the side-chain steps
  uint8_t* lflag;      // [n]
  uint8_t* mflag;      // [n_mov]
};

// the per-atom part of the plan, bounded by DDP_MINIMIZE_FLEX_MAX_STATE_BYTES, and the whole dynamic LDS block
static inline size_t fx_state_bytes(int n, int n_mov, int n_sc) { return (size_t)89 * n + (size_t)81 * n_mov + (size_t)4 * n_sc; }
static inline size_t fx_lds_bytes(int n, int n_mov, int n_sc) { return DDP_FX_FIXED_BYTES + fx_state_bytes(n, n_mov, n_sc); }

// host: what ddp_pose_minimize_flex and ddp_pose_search_flex check alike before they look at their own pointers: the shape, the limits
// of the plan (DDP_ELIMIT) and the side-chain tables
static inline int fx_check(const char* who, const ddp_minimize_flex_args_t* a) {
  if (const int rc = ddp_pose_check_shape(who, a->n_samples, a->n, a->m, a->rec_stride,
                                          a->n_tor >= 0 && a->n_mov >= 0 && a->n_sc >= 0 && a->n_sub >= 0, true))
    return rc;
  if (const int rc = DDP_POSE_CHECK_ATOMS(who, a->n, DDP_MINIMIZE_MAX_ATOMS)) return rc;
  if (a->n_tor > DDP_MINIMIZE_MAX_TORSIONS) {
    char msg[128];
    snprintf(msg, sizeof msg, "%s: more than DDP_MINIMIZE_MAX_TORSIONS rotatable bonds", who);
    return ddp_fail(DDP_ELIMIT, msg);
  }
  return DDP_POSE_CHECK_SIDECHAINS(who, a, DDP_MINIMIZE_FLEX_MAX_MOVING, DDP_MINIMIZE_FLEX_MAX_BONDS, fx_state_bytes(a->n, a->n_mov, a->n_sc),
                                   DDP_MINIMIZE_FLEX_MAX_STATE_BYTES, "DDP_MINIMIZE_FLEX_MAX_STATE_BYTES");
}

__device__ __forceinline__ FxLds fx_carve(unsigned char* p, int n, int n_mov, int n_sc) {
  FxLds L;
  L.tile = (float4*)p; p += DDP_FX_TILE * sizeof(float4);
  L.tflag = p; p += DDP_FX_TILE;
  L.we = (double(*)[8])p; L.wr = (double*)p + DDP_FX_WAVES * 8; p += DDP_FX_WE_BYTES;
  L.red = (double*)p; p += DDP_FX_RED_BYTES;
  L.et = (double*)p; p += 64;
  L.we2 = (double(*)[4])p; L.wr2 = (double*)p + DDP_FX_WAVES * 4; p += DDP_FX_WE2_BYTES;
  L.g = (double*)p; p += (size_t)48 * n;
  L.gm = (double*)p; p += (size_t)48 * n_mov;
  L.x = (float*)p; p += (size_t)24 * n;
  L.ym = (float*)p; p += (size_t)24 * n_mov;
  L.rg = (float*)p; p += (size_t)12 * n;
  L.rad = (float*)p; p += (size_t)4 * n;
  L.mrad = (float*)p; p += (size_t)4 * n_mov;
  L.mov = (int32_t*)p; p += (size_t)4 * n_mov;
  L.scstep = (float*)p; p += (size_t)4 * n_sc;
  L.lflag = p; p += n;
  L.mflag = p;
  return L;
}

// the tables of the plan: the ligand's radii and flags, the moving atoms' receptor indices, radii and flags.  An index outside the
// receptor: no read, the atom takes part in nothing.  Visible after the caller's next barrier.  Args: ddp_minimize_flex_args_t, or the
// struct of another entry with the same field names (ddp_score_guidance_flex_args_t).
template <class Args>
__device__ __forceinline__ void fx_load_tables(const Args& A, const FxLds& L) {
  const int tid = threadIdx.x, n = A.n, m = A.m, n_mov = A.n_mov;
  for (int i = tid; i < n; i += DDP_FX_THREADS) { L.rad[i] = A.lig_radii[i]; L.lflag[i] = A.lig_flags[i]; }
  for (int r = tid; r < n_mov; r += DDP_FX_THREADS) {
    const int a = A.mov[r];
    const bool in = a >= 0 && a < m;
    L.mov[r] = a;
    L.mrad[r] = in ? A.rec_radii[a] : -1.f;
    L.mflag[r] = in ? A.rec_flags[a] : (uint8_t)0;
  }
}

// slot of receptor atom a among the moving atoms (mov sorted), or -1
__device__ __forceinline__ int fx_slot(const int32_t* mov, int n_mov, int a) {
  int lo = 0, hi = n_mov;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (mov[mid] < a) lo = mid + 1;
    else hi = mid;
  }
  return (lo < n_mov && mov[lo] == a) ? lo : -1;
}

// the tile-load hook of score_evaluate: a moving atom comes from ym (LDS), not from global memory
struct FxPatch {
  const int32_t* mov;
  int n_mov;
  const float* ym;
  __device__ __forceinline__ void operator()(int j, float4& r, uint8_t& f) const {
    const int k = fx_slot(mov, n_mov, j);
    if (k >= 0) {
      r.x = ym[3 * k]; r.y = ym[3 * k + 1]; r.z = ym[3 * k + 2];
      f |= DDP_FX_MOVING;
    }
  }
};

// coordinates of receptor atom a (inside [0, m)): the moving atoms' LDS copy ym or the sample's receptor in global memory
__device__ __forceinline__ void fx_atom(const FxLds& L, int n_mov, const float* rs, const float* ym, int a, float* p) {
  const int k = fx_slot(L.mov, n_mov, a);
  if (k >= 0) { p[0] = ym[3 * k]; p[1] = ym[3 * k + 1]; p[2] = ym[3 * k + 2]; }
  else { p[0] = rs[3 * a]; p[1] = rs[3 * a + 1]; p[2] = rs[3 * a + 2]; }
}

// The second pass of one evaluation, for the state (x, ym) in LDS with the receptor tile of score_evaluate (patched by FxPatch) still in
// L.tile when m <= one tile: gm = d inter / dy_a + d sc / dy_a of every moving atom (lane 0 of the owning wave: visible after the
// caller's next barrier) and L.we2 = the waves' partial sums of the four unweighted sc terms.  Shared by fx_evaluate below and by
// ddp_score_guidance_flex_kernel (ddp_score_guidance_flex.hip).  Args as fx_load_tables.
template <class Args>
__device__ __forceinline__ void fx_second_pass(const Args& A, const FxLds& L, const float* rs, const float* x, const float* ym, double* gm) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = A.n, m = A.m, n_mov = A.n_mov;
  const FxPatch patch = {L.mov, n_mov, ym};
  // d inter / dy_a by gather over the ligand atoms; the assignment also clears gm
  const ddp_score_form_t& F = A.form;
  const double cut2 = F.cutoff * F.cutoff;
  for (int r = wave; r < n_mov; r += DDP_FX_WAVES) {
    ScoreAcc acc = {{0.0, 0.0, 0.0, 0.0}, 0.0, 0.0, 0.0};     // (its energy sums are not used: step 1 has them)
    const double ra = L.mrad[r];
    if (ra >= 0.0) {                               // (wave-uniform, no barrier inside)
      const double xa = ym[3 * r], ya = ym[3 * r + 1], za = ym[3 * r + 2];
      const unsigned fa = L.mflag[r];
      for (int i = lane; i < n; i += 64) {
        if (L.rad[i] < 0.f) continue;
        score_pair<true>(F, cut2, xa - (double)x[3 * i], ya - (double)x[3 * i + 1], za - (double)x[3 * i + 2], ra + (double)L.rad[i], fa,
                         L.lflag[i], acc);
      }
    }
    const double gx = wave_sum(acc.gx), gy = wave_sum(acc.gy), gz = wave_sum(acc.gz);
    if (lane == 0) { gm[3 * r] = gx; gm[3 * r + 1] = gy; gm[3 * r + 2] = gz; }   // (atom r is this wave's alone)
  }
  // sc: the partners of sc_pairs, tile by tile.  st: partners that stay, mv: partners that move themselves (half the energy)
  ScoreAcc st = {{0.0, 0.0, 0.0, 0.0}, 0.0, 0.0, 0.0}, mv = {{0.0, 0.0, 0.0, 0.0}, 0.0, 0.0, 0.0};
  for (int j0 = 0; n_mov > 0 && j0 < m; j0 += DDP_FX_TILE) {
    const int mt = min(DDP_FX_TILE, m - j0);
    if (m > DDP_FX_TILE) {                         // (the same for all threads) more than one tile: stream them again
      __syncthreads();
      for (int j = tid; j < mt; j += DDP_FX_THREADS) {
        float4 q = make_float4(rs[3 * (j0 + j)], rs[3 * (j0 + j) + 1], rs[3 * (j0 + j) + 2], A.rec_radii[j0 + j]);
        uint8_t f = A.rec_flags[j0 + j];
        patch(j0 + j, q, f);
        L.tile[j] = q;
        L.tflag[j] = f;
      }
      __syncthreads();
    }
    for (int r = wave; r < n_mov; r += DDP_FX_WAVES) {
      const double ra = L.mrad[r];
      st.gx = st.gy = st.gz = 0.0;
      mv.gx = mv.gy = mv.gz = 0.0;
      if (ra >= 0.0) {
        const double xa = ym[3 * r], ya = ym[3 * r + 1], za = ym[3 * r + 2];
        const unsigned fa = L.mflag[r];
        const int a = L.mov[r];
        const uint8_t* __restrict__ sp = A.sc_pairs + (size_t)r * m + j0;
        for (int j = lane; j < mt; j += 64) {
          if (!sp[j] || j0 + j == a) continue;
          const float4 q = L.tile[j];
          if (q.w < 0.f) continue;                 // an untyped receptor atom
          const unsigned fj = L.tflag[j];
          const double dx = xa - (double)q.x, dy = ya - (double)q.y, dz = za - (double)q.z, rsum = ra + (double)q.w;
          if (fj & DDP_FX_MOVING) score_pair<true>(F, cut2, dx, dy, dz, rsum, fa, fj, mv);
          else score_pair<true>(F, cut2, dx, dy, dz, rsum, fa, fj, st);
        }
      }
      const double gx = wave_sum(st.gx + mv.gx), gy = wave_sum(st.gy + mv.gy), gz = wave_sum(st.gz + mv.gz);
      if (lane == 0) { gm[3 * r] += gx; gm[3 * r + 1] += gy; gm[3 * r + 2] += gz; }
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double c = wave_sum(st.t[k]) + 0.5 * wave_sum(mv.t[k]);
    if (lane == 0) L.we2[wave][k] = c;
  }
}

// by one thread, after the barrier behind fx_second_pass: sc = the weighted sum of the four terms, the waves in wave order
__device__ __forceinline__ double fx_sc_total(const ddp_score_form_t& F, const double (*we2)[4]) {
  double c[4];
  for (int k = 0; k < 4; ++k) {
    c[k] = we2[0][k];
    for (int w = 1; w < DDP_FX_WAVES; ++w) c[k] += we2[w][k];
  }
  return F.w_gauss * c[0] + F.w_repulsion * c[1] + F.w_hydrophobic * c[2] + F.w_hbond * c[3];
}

// Energy [inter, intra, sc, ligand restraint term, side-chain restraint term, E] -> L.et, gradients -> g and gm of the state (x, ym)
// (LDS, visible to all threads on entry).  Ends with a barrier: L.et, g and gm are visible on return.
__device__ __forceinline__ void fx_evaluate(const ddp_minimize_flex_args_t& A, const FxLds& L, const float* rs, const float* __restrict__ as,
                                         const float* __restrict__ ras, const float* x, const float* ym, double* g, double* gm) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = A.n, m = A.m, n_mov = A.n_mov;
  const FxPatch patch = {L.mov, n_mov, ym};
  score_evaluate<true>(A, rs, L.tile, L.tflag, x, L.rad, L.lflag, g, L.we, patch);
  descent_ligand_restraint(A, x, as, g, L.wr);
  fx_second_pass(A, L, rs, x, ym, gm);
  // the side-chain restraint
  const double krs = n_mov > 0 ? 2.0 * A.restraint_sc / (double)n_mov : 0.0;
  double er2_w = 0.0;
  for (int r = wave; r < n_mov; r += DDP_FX_WAVES) {
    const int a = L.mov[r];
    if (a < 0 || a >= m) continue;                 // an index outside the receptor: no read (wave-uniform)
    const double ax = (double)ym[3 * r] - (double)ras[3 * a], ay = (double)ym[3 * r + 1] - (double)ras[3 * a + 1],
                 az = (double)ym[3 * r + 2] - (double)ras[3 * a + 2];
    er2_w += ax * ax + ay * ay + az * az;
    if (lane == 0) { gm[3 * r] = gm[3 * r] + krs * ax; gm[3 * r + 1] = gm[3 * r + 1] + krs * ay; gm[3 * r + 2] = gm[3 * r + 2] + krs * az; }
  }
  if (lane == 0) L.wr2[wave] = er2_w;
  __syncthreads();
  if (tid == 0) {
    double t[8], inter, intra, er = L.wr[0], er2 = L.wr2[0];
    score_totals(A.form, L.we, t, inter, intra);
    for (int w = 1; w < DDP_FX_WAVES; ++w) { er += L.wr[w]; er2 += L.wr2[w]; }
    const double sc = fx_sc_total(A.form, L.we2);
    const double rest = A.restraint * (er / (double)n);
    const double rest2 = n_mov > 0 ? A.restraint_sc * (er2 / (double)n_mov) : 0.0;
    L.et[0] = inter; L.et[1] = intra; L.et[2] = sc; L.et[3] = rest; L.et[4] = rest2;
    L.et[5] = (((inter + intra) + sc) + rest) + rest2;
  }
  __syncthreads();
}

// the range of sc_sub that bond j turns, clamped to the table
template <class Args>
__device__ __forceinline__ void fx_range(const Args& A, int j, int& m0, int& m1) {
  m0 = min(max(A.sc_map[2 * j], 0), A.n_sub);
  m1 = min(max(A.sc_map[2 * j + 1], 0), A.n_sub);
}

// L.scstep[j] = step * the inertia-scaled direction of side-chain bond j at the state ym with the gradient gm, fp64, rounded to fp32.
// Wave w owns the bonds w, w + 4, ..., its lanes stride over the bond's subcomponent.  Visible after the caller's next barrier.
// Args as fx_load_tables.
template <class Args>
__device__ __forceinline__ void fx_sc_direction(const Args& A, const FxLds& L, const float* rs, const float* ym, const double* gm, double step) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, m = A.m, n_mov = A.n_mov;
  for (int j = wave; j < A.n_sc; j += DDP_FX_WAVES) {
    const int u = A.sc_edge_idx[2 * j], v = A.sc_edge_idx[2 * j + 1];
    double num = 0.0, den = 0.0;
    if (u >= 0 && u < m && v >= 0 && v < m) {      // an entry outside the receptor: no read, the bond gets 0
      float pu[3], pv[3];
      fx_atom(L, n_mov, rs, ym, u, pu);
      fx_atom(L, n_mov, rs, ym, v, pv);
      const double vx = pv[0], vy = pv[1], vz = pv[2];
      double ux = (double)pu[0] - vx, uy = (double)pu[1] - vy, uz = (double)pu[2] - vz;
      const double len = sqrt(ux * ux + uy * uy + uz * uz);
      ux /= len; uy /= len; uz /= len;
      int m0, m1;
      fx_range(A, j, m0, m1);
      for (int i = m0 + lane; i < m1; i += 64) {
        const int a = A.sc_sub[i];
        if (a < 0 || a >= m || a == u || a == v) continue;   // the bond's own atoms lie on the axis: no lever, exactly
        const int k = fx_slot(L.mov, n_mov, a);
        if (k < 0) continue;                       // not a moving atom: it takes part in nothing
        const double px = (double)ym[3 * k] - vx, py = (double)ym[3 * k + 1] - vy, pz = (double)ym[3 * k + 2] - vz;
        const double ax = uy * pz - uz * py, ay = uz * px - ux * pz, az = ux * py - uy * px;
        num += gm[3 * k] * ax + gm[3 * k + 1] * ay + gm[3 * k + 2] * az;
        den += ax * ax + ay * ay + az * az;
      }
    }
    num = wave_sum(num); den = wave_sum(den);
    if (lane == 0) L.scstep[j] = (float)(step * (den == 0.0 ? 0.0 : -num / den));
  }
}

// yt = the side-chain map of ddp_sidechain_update_kernel applied to ym with the angles L.scstep, fp32, bonds in list order; the axis of a
// bond is read by every thread before the barrier behind which the bond's atoms move.  Ends with a barrier: yt is visible on return.
__device__ __forceinline__ void fx_sc_update(const ddp_minimize_flex_args_t& A, const FxLds& L, const float* rs, const float* ym, float* yt) {
  const int tid = threadIdx.x, m = A.m, n_mov = A.n_mov;
  for (int i = tid; i < 3 * n_mov; i += DDP_FX_THREADS) yt[i] = ym[i];
  __syncthreads();
  float M[9];
  for (int j = 0; j < A.n_sc; ++j) {
    const int u = A.sc_edge_idx[2 * j], v = A.sc_edge_idx[2 * j + 1];
    if (u < 0 || u >= m || v < 0 || v >= m) continue;   // an entry outside the receptor: no read, no rotation (the same for all threads)
    float pu[3], pv[3];
    fx_atom(L, n_mov, rs, yt, u, pu);
    fx_atom(L, n_mov, rs, yt, v, pv);
    const float ax = pu[0] - pv[0], ay = pu[1] - pv[1], az = pu[2] - pv[2];
    const float k = L.scstep[j] / sqrtf(ax * ax + ay * ay + az * az);
    rotvec_to_matrix(ax * k, ay * k, az * k, M);
    __syncthreads();                             // every thread has read the axis before an atom on it may move
    int m0, m1;
    fx_range(A, j, m0, m1);
    for (int i = m0 + tid; i < m1; i += DDP_FX_THREADS) {
      const int a = A.sc_sub[i];
      if (a < 0 || a >= m) continue;
      const int s = fx_slot(L.mov, n_mov, a);
      if (s < 0) continue;
      const float px = yt[3 * s] - pv[0], py = yt[3 * s + 1] - pv[1], pz = yt[3 * s + 2] - pv[2];
      yt[3 * s] = M[0] * px + M[1] * py + M[2] * pz + pv[0];
      yt[3 * s + 1] = M[3] * px + M[4] * py + M[5] * pz + pv[1];
      yt[3 * s + 2] = M[6] * px + M[7] * py + M[8] * pz + pv[2];
    }
    __syncthreads();
  }
}

// `iterations` iterations of the joint line search, the counterpart of mz_descend.  On entry the start state lies in the TRIAL
// buffers L.x + (cur ^ 1) 3 n and L.ym + (cur ^ 1) 3 n_mov (the moving atoms come from wherever the caller read them: the sample's
// receptor or a row's own state) and the tables of fx_load_tables are in place, all visible (a barrier behind them); pass 0 of the
// loop evaluates the start state and takes it whatever its energy.  On return the state lies in L.x + cur 3 n / L.ym + cur 3 n_mov
// and its gradients in L.g / L.gm at the same offsets (cur has flipped once per state taken), e[6] holds its energies and e0[6]
// those of the start state, step and taken have been advanced; every thread holds the same values, read from the same LDS words.
// hist (or NULL): thread 0 writes E before the first and after every iteration to hist[it hist_stride].  rs: the row's receptor
// (global memory; its moving atoms are never read here), as / ras: the anchors of ligand and receptor.  There is exactly ONE call
// site of the evaluation.  No data-dependent control flow around a barrier: the trip count is an argument, the accept decision
// follows the last barrier of the evaluation.
__device__ __forceinline__ void fx_descend(const ddp_minimize_flex_args_t& A, const FxLds& L, const float* rs, const float* __restrict__ as,
                                           const float* __restrict__ ras, int iterations, int& cur, double& step, int& taken, double* e,
                                           double* e0, double* hist, size_t hist_stride) {
  const int tid = threadIdx.x, n = A.n, n_mov = A.n_mov;
  for (int it = 0; it <= iterations; ++it) {
    if (it > 0) {
      // the ligand torsion steps go to the tile's first n_tor floats, the side-chain steps to L.scstep; the barrier makes them visible
      float tr[3], rot[3];
      descent_direction<true>(L.x + cur * 3 * n, L.g + cur * 3 * n, n, A.n_tor, A.bonds, A.mask_rotate, step, L.red, tr, rot, (float*)L.tile);
      fx_sc_direction(A, L, rs, L.ym + cur * 3 * n_mov, L.gm + cur * 3 * n_mov, step);
      __syncthreads();
      descent_pose_update(A, L.x + cur * 3 * n, L.x + (cur ^ 1) * 3 * n, L.rg, (const float*)L.tile, (float*)L.red, tr, rot);
      fx_sc_update(A, L, rs, L.ym + cur * 3 * n_mov, L.ym + (cur ^ 1) * 3 * n_mov);
    }
    fx_evaluate(A, L, rs, as, ras, L.x + (cur ^ 1) * 3 * n, L.ym + (cur ^ 1) * 3 * n_mov, L.g + (cur ^ 1) * 3 * n, L.gm + (cur ^ 1) * 3 * n_mov);
    const double et5 = L.et[5];
    const bool take = it == 0 || et5 < e[5];     // strict, fp64, false for NaN; the same LDS words for every thread
    if (take) {
      e[0] = L.et[0]; e[1] = L.et[1]; e[2] = L.et[2]; e[3] = L.et[3]; e[4] = L.et[4]; e[5] = et5;
      cur ^= 1;
    }
    if (it > 0) {
      step = take ? fmin(A.grow * step, A.step_max) : A.shrink * step;
      taken += take ? 1 : 0;
    } else {
      for (int k = 0; k < 6; ++k) e0[k] = e[k];
    }
    if (hist && tid == 0) hist[(size_t)it * hist_stride] = e[5];
    // (the next write of L.et lies behind the barriers of the next evaluation)
  }
}

#endif
