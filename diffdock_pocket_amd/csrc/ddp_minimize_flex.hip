// ddp_minimize_flex.hip - local minimisation of sampled poses TOGETHER with the flexible side chains of their receptor, the whole line
// search of a pose in ONE launch (include/ddp_hip.h, ddp_pose_minimize_flex; host side diffdock_pocket_amd/minimize_flex.py, which
// states the whole definition).  The sibling of ddp_minimize.hip: the same loop, the same accept rule, the same one call site of the
// evaluation, with a second molecule in the state.  One 256-thread workgroup per pose holds, for the whole call, what ddp_pose_minimize
// holds for the ligand and, for the n_mov moving receptor atoms, the current and the trial coordinates, both gradients, radii, flags,
// their receptor indices and the side-chain steps.  The LDS plan, the evaluation and the loop (fx_descend) live in
// ddp_minimize_flex_loop.h, which ddp_search_flex.hip shares; this file is the kernel around them and the host entry (fx_check of that
// header holds the checks the two entries share).
// The evaluation (its three passes, the fixed order of every sum, what keeps control flow uniform around the barriers) is described at
// the head of that header.
#include "ddp_minimize_flex_loop.h"

__global__ __launch_bounds__(DDP_FX_THREADS) void ddp_pose_minimize_flex_kernel(const ddp_minimize_flex_args_t A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char fx_lds[];
  const int s = blockIdx.x, tid = threadIdx.x, n = A.n, m = A.m, n_mov = A.n_mov, S = A.n_samples;
  const FxLds L = fx_carve(fx_lds, n, n_mov, A.n_sc);
  float* gpos = A.pos + (size_t)s * n * 3;
  const float* __restrict__ as = A.anchor + (size_t)s * n * 3;
  float* rs = A.rec + (size_t)s * A.rec_stride;      // read through the whole call, its moving atoms written once at exit
  const float* __restrict__ ras = A.rec_anchor + (size_t)s * A.rec_stride;
  // the start state goes into the TRIAL buffers: pass 0 of the loop evaluates it and takes it whatever its energy
  int cur = 0;
  for (int i = tid; i < 3 * n; i += DDP_FX_THREADS) L.x[3 * n + i] = gpos[i];
  fx_load_tables(A, L);
  for (int r = tid; r < n_mov; r += DDP_FX_THREADS) {
    const int a = A.mov[r];
    const bool in = a >= 0 && a < m;               // an index outside the receptor: no read, the atom takes part in nothing
    float* y = L.ym + 3 * n_mov + 3 * r;
    y[0] = in ? rs[3 * a] : 0.f; y[1] = in ? rs[3 * a + 1] : 0.f; y[2] = in ? rs[3 * a + 2] : 0.f;
  }
  double step = A.step[s];
  int taken = 0;
  double e[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, e0[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  __syncthreads();
  fx_descend(A, L, rs, as, ras, A.iterations, cur, step, taken, e, e0, A.history ? A.history + s : (double*)nullptr, (size_t)S);
  if (tid == 0) {
    double* ei = A.energy_in + 6 * (size_t)s;
    for (int k = 0; k < 6; ++k) ei[k] = e0[k];
  }
  if (tid == 0) {
    double* eo = A.energy_out + 6 * (size_t)s;
    for (int k = 0; k < 6; ++k) eo[k] = e[k];
  }
  if (A.iterations > 0 && tid == 0) { A.step[s] = step; A.accepted[s] += taken; }
  if (taken > 0) {
    for (int i = tid; i < 3 * n; i += DDP_FX_THREADS) gpos[i] = L.x[cur * 3 * n + i];
    for (int r = tid; r < n_mov; r += DDP_FX_THREADS) {
      const int a = L.mov[r];
      if (a < 0 || a >= m) continue;
      const float* y = L.ym + cur * 3 * n_mov + 3 * r;
      rs[3 * a] = y[0]; rs[3 * a + 1] = y[1]; rs[3 * a + 2] = y[2];
    }
  }
  if (A.grad) {
    double* go = A.grad + (size_t)s * n * 3;
    for (int i = tid; i < 3 * n; i += DDP_FX_THREADS) go[i] = L.g[cur * 3 * n + i];
  }
  if (A.grad_mov) {
    double* go = A.grad_mov + (size_t)s * n_mov * 3;
    for (int i = tid; i < 3 * n_mov; i += DDP_FX_THREADS) go[i] = L.gm[cur * 3 * n_mov + i];
  }
}

extern "C" int ddp_pose_minimize_flex(const ddp_minimize_flex_args_t* a, void* stream) {
  if (!a) return ddp_fail(DDP_EINVAL, "ddp_pose_minimize_flex: null argument struct");
  if (a->n_samples == 0) return 0;
  if (const int rc = fx_check("ddp_pose_minimize_flex", a)) return rc;
  if (!a->pos || !a->anchor || !a->lig_radii || !a->lig_flags || !a->step || !a->accepted || !a->energy_in || !a->energy_out ||
      (a->m > 0 && (!a->rec || !a->rec_radii || !a->rec_flags)) || (a->n_tor > 0 && (!a->bonds || !a->mask_rotate)) ||
      (a->n_mov > 0 && !a->rec_anchor))
    return ddp_fail(DDP_EINVAL, "ddp_pose_minimize_flex: null argument");
  if (a->iterations < 0 || !(a->restraint >= 0.0) || !(a->restraint_sc >= 0.0))
    return ddp_fail(DDP_EINVAL, "ddp_pose_minimize_flex: iterations or a restraint < 0");
  if (const int rc = score_check_constants(&a->form, "ddp_pose_minimize_flex")) return rc;
  // 18496 bytes fixed + 89 per ligand atom + 81 per moving atom + 4 per side-chain bond: at most 64 KiB
  hipLaunchKernelGGL(ddp_pose_minimize_flex_kernel, dim3(a->n_samples), dim3(DDP_FX_THREADS), fx_lds_bytes(a->n, a->n_mov, a->n_sc),
                     (hipStream_t)stream, *a);
  return ddp_launch_result("ddp_pose_minimize_flex");
}
