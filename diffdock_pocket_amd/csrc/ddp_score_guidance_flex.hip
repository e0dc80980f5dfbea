// ddp_score_guidance_flex.hip - the physics-score guidance term of the reverse-diffusion step with the flexible side chains guided too
// (include/ddp_hip.h, ddp_score_guidance_flex; host side diffdock_pocket_amd/score_guidance.py, which states the definition, and
// sampler.py).  In a flexible run with score_guidance_sidechains it replaces the ddp_score_guidance launch of the step: one launch,
// one 256-thread workgroup per sample, the shape of ddp_score_guidance_kernel, and both jobs.  For sample s with the fp32 pose x the
// scores were computed for and y its current receptor atoms, E(x, y) = inter(x, y) + intra(x) + sc(y) is the joint energy of
// ddp_pose_minimize_flex at both restraints 0:
//   1. score_evaluate<true> of ddp_pose_descent.h leaves dE/dx in LDS; FxPatch marks the moving atoms in the tile as the minimiser's
//      evaluation does (their coordinates are the receptor's own: the patch writes the same bits back).  No restraint term is added to
//      the gradient, so the ligand increments are those of ddp_score_guidance bit for bit.
//   2. fx_second_pass of ddp_minimize_flex_loop.h, the code ddp_pose_minimize_flex runs: d inter/dy by gather over the ligand in LDS,
//      then the energy and gradient of sc over sc_pairs, tile by tile.  No atomics.
//   3. the ligand increments exactly as ddp_score_guidance_kernel: descent_direction, the block maximum, f_s, upd[0 .. 2].
//   4. fx_sc_direction for step = w: d_sc[j] in fp64, rounded to fp32; one more block maximum; f_sc = min(1, max_sc / max_j |d_sc[j]|)
//      in fp64 (a zero maximum: no constraint); upd_sc[s][j] += (float)(f_sc * (double)d_sc[j]), every element by one thread.
// Every sum has a fixed order: two launches give the same bits.  No data-dependent control flow around a barrier: the early return on
// !(w > 0) is the same for all threads of all workgroups and is the only exit; trip counts and the condition that skips the tile reload
// (m <= one tile) are kernel arguments.  The receptor is only read.  A NaN poisons its own sample only (no value crosses workgroups).
#include "ddp_minimize_flex_loop.h"

// The dynamic LDS: the fixed part of ddp_minimize_flex_loop.h (tile, tile flags, partial sums, block-sum scratch), then ONE copy of the
// state in the order of the carve below: fp64 (both gradients), fp32 (pose, moving atoms, radii, indices, the two directions), bytes.
#define SGF_STATE_BYTES(n, n_mov, n_sc, n_tor) ((size_t)41 * (n) + (size_t)45 * (n_mov) + (size_t)4 * (n_sc) + (size_t)4 * (n_tor) + 32)
#define SGF_LDS_BYTES(n, n_mov, n_sc, n_tor) (DDP_FX_FIXED_BYTES + SGF_STATE_BYTES(n, n_mov, n_sc, n_tor))
static_assert(SGF_LDS_BYTES(DDP_SCORE_GUIDANCE_FLEX_MAX_ATOMS, DDP_SCORE_GUIDANCE_FLEX_MAX_MOVING, DDP_SCORE_GUIDANCE_FLEX_MAX_BONDS,
                            DDP_SCORE_GUIDANCE_FLEX_MAX_TORSIONS) <= 64 * 1024,
              "ddp_score_guidance_flex: the LDS plan must fit the 64 KiB a workgroup gets without opting in to more");
static_assert(SGF_LDS_BYTES(DDP_SCORE_GUIDANCE_FLEX_MAX_ATOMS, DDP_SCORE_GUIDANCE_FLEX_MAX_MOVING, DDP_SCORE_GUIDANCE_FLEX_MAX_BONDS,
                            DDP_SCORE_GUIDANCE_FLEX_MAX_TORSIONS) == 56160, "the header states the plan at the limits");
static_assert(DDP_DESCENT_WAVES * 6 * 8 <= DDP_FX_RED_BYTES, "descent_direction's block sums fit the scratch");

__global__ __launch_bounds__(DDP_FX_THREADS) void ddp_score_guidance_flex_kernel(const ddp_score_guidance_flex_args_t A) {
  const float w = *A.weight;
  if (!(w > 0.f)) return;                                 // (the same for all threads and all workgroups) nothing is stored
  extern __shared__ __attribute__((aligned(16))) unsigned char sgf_lds[];
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = A.n, m = A.m, T = A.n_tor, n_mov = A.n_mov, n_sc = A.n_sc;
  FxLds L = {};
  unsigned char* p = sgf_lds;
  L.tile = (float4*)p; p += DDP_FX_TILE * sizeof(float4);
  L.tflag = p; p += DDP_FX_TILE;
  L.we = (double(*)[8])p; p += DDP_FX_WE_BYTES;
  L.red = (double*)p; p += DDP_FX_RED_BYTES + 64;        // (the 64 bytes of the minimiser's energies are not used here)
  L.we2 = (double(*)[4])p; p += DDP_FX_WE2_BYTES;
  L.g = (double*)p; p += (size_t)24 * n;
  L.gm = (double*)p; p += (size_t)24 * n_mov;
  L.x = (float*)p; p += (size_t)12 * n;
  L.ym = (float*)p; p += (size_t)12 * n_mov;
  L.rad = (float*)p; p += (size_t)4 * n;
  L.mrad = (float*)p; p += (size_t)4 * n_mov;
  L.mov = (int32_t*)p; p += (size_t)4 * n_mov;
  L.scstep = (float*)p; p += (size_t)4 * n_sc;           // d_sc
  float* tor = (float*)p; p += (size_t)4 * T;            // d_tor
  float* dir = (float*)p; p += 32;                       // d_tr [3], d_rot [3] (+ 2 unused)
  L.lflag = p; p += n;
  L.mflag = p;
  const float* __restrict__ rs = A.rec + (size_t)s * A.rec_stride;
  const float* __restrict__ ls = A.pos + (size_t)s * n * 3;
  for (int i = tid; i < 3 * n; i += DDP_FX_THREADS) L.x[i] = ls[i];
  fx_load_tables(A, L);
  for (int r = tid; r < n_mov; r += DDP_FX_THREADS) {
    const int a = A.mov[r];
    const bool in = a >= 0 && a < m;                      // an index outside the receptor: no read, the atom takes part in nothing
    float* y = L.ym + 3 * r;
    y[0] = in ? rs[3 * a] : 0.f; y[1] = in ? rs[3 * a + 1] : 0.f; y[2] = in ? rs[3 * a + 2] : 0.f;
  }
  __syncthreads();
  const FxPatch patch = {L.mov, n_mov, L.ym};
  score_evaluate<true>(A, rs, L.tile, L.tflag, L.x, L.rad, L.lflag, L.g, L.we, patch);   // ends with a barrier
  fx_second_pass(A, L, rs, L.x, L.ym, L.gm);
  __syncthreads();                                        // gm and we2 (lane 0 of the owning waves) are visible
  if (A.grad_mov) {
    double* go = A.grad_mov + (size_t)s * n_mov * 3;
    for (int i = tid; i < 3 * n_mov; i += DDP_FX_THREADS) go[i] = L.gm[i];
  }
  if (A.energy && tid == 0) {
    double t[8], inter, intra;
    score_totals(A.form, L.we, t, inter, intra);
    double* e = A.energy + 3 * (size_t)s;
    e[0] = inter; e[1] = intra; e[2] = fx_sc_total(A.form, L.we2);
  }
  // ---- the ligand increments, as ddp_score_guidance_kernel
  double* red = L.red;
  descent_direction<false>(L.x, L.g, n, T, A.bonds, A.mask_rotate, (double)w, red, dir, dir + 3, tor);
  fx_sc_direction(A, L, rs, L.ym, L.gm, (double)w);      // (touches neither red nor dir nor tor)
  __syncthreads();                                        // dir (thread 0), tor and d_sc (lane 0 of the owning waves) are visible
  double mx = 0.0, ms = 0.0;
  for (int b = tid; b < T; b += DDP_FX_THREADS) mx = fmax(mx, fabs((double)tor[b]));
  for (int j = tid; j < n_sc; j += DDP_FX_THREADS) ms = fmax(ms, fabs((double)L.scstep[j]));
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { mx = fmax(mx, __shfl_xor(mx, off)); ms = fmax(ms, __shfl_xor(ms, off)); }
  if (lane == 0) { red[wave] = mx; red[DDP_FX_WAVES + wave] = ms; }   // (red's last readers passed the barrier above)
  __syncthreads();
  mx = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
  ms = fmax(fmax(red[4], red[5]), fmax(red[6], red[7]));
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
    for (int b = tid; b < T; b += DDP_FX_THREADS) u[b] = u[b] + (float)(f * (double)tor[b]);
  }
  // ---- the side-chain increments: a cap factor of their own
  if (n_sc > 0) {
    const double fs = ms > 0.0 ? fmin(1.0, A.max_sc / ms) : 1.0;
    float* u = A.upd_sc + (size_t)s * n_sc;
    for (int j = tid; j < n_sc; j += DDP_FX_THREADS) u[j] = u[j] + (float)(fs * (double)L.scstep[j]);
  }
}

extern "C" int ddp_score_guidance_flex(const ddp_score_guidance_flex_args_t* a, void* stream) {
  const char* who = "ddp_score_guidance_flex";
  if (!a) return ddp_fail(DDP_EINVAL, "ddp_score_guidance_flex: null argument struct");
  if (a->n_samples == 0) return 0;
  if (const int rc = ddp_pose_check_shape(who, a->n_samples, a->n, a->m, a->rec_stride,
                                          a->n_tor >= 0 && a->n_mov >= 0 && a->n_sc >= 0 && a->n_sub >= 0, true))
    return rc;
  if (const int rc = DDP_POSE_CHECK_ATOMS(who, a->n, DDP_SCORE_GUIDANCE_FLEX_MAX_ATOMS)) return rc;
  if (a->n_tor > DDP_SCORE_GUIDANCE_FLEX_MAX_TORSIONS)
    return ddp_fail(DDP_ELIMIT, "ddp_score_guidance_flex: more than DDP_SCORE_GUIDANCE_FLEX_MAX_TORSIONS rotatable bonds");
  if (const int rc = DDP_POSE_CHECK_SIDECHAINS(who, a, DDP_SCORE_GUIDANCE_FLEX_MAX_MOVING, DDP_SCORE_GUIDANCE_FLEX_MAX_BONDS, 0, 0, nullptr))
    return rc;
  if (!a->pos || !a->lig_radii || !a->lig_flags || !a->weight || !a->upd[0] || !a->upd[1] ||
      (a->m > 0 && (!a->rec || !a->rec_radii || !a->rec_flags)) || (a->n_tor > 0 && (!a->bonds || !a->mask_rotate || !a->upd[2])) ||
      (a->n_sc > 0 && !a->upd_sc))
    return ddp_fail(DDP_EINVAL, "ddp_score_guidance_flex: null argument");
  if (const int rc = score_check_constants(&a->form, who)) return rc;
  if (!(a->max_tr >= 0.0) || !(a->max_rot >= 0.0) || !(a->max_tor >= 0.0) || !(a->max_sc >= 0.0))
    return ddp_fail(DDP_EINVAL, "ddp_score_guidance_flex: the caps must not be negative or NaN");
  hipLaunchKernelGGL(ddp_score_guidance_flex_kernel, dim3(a->n_samples), dim3(DDP_FX_THREADS),
                     SGF_LDS_BYTES(a->n, a->n_mov, a->n_sc, a->n_tor), (hipStream_t)stream, *a);
  return ddp_launch_result(who);
}
