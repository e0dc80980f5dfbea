// ddp_internal.h - shared helpers of libddp_hip.so (not part of the C ABI).
#ifndef DDP_INTERNAL_H
#define DDP_INTERNAL_H
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "ddp_hip.h"

int ddp_fail(int code, const char* msg);
int ddp_fail_hip(hipError_t err, const char* where);

// ---- host: what the entries over "n_samples poses of one ligand against a receptor" check alike, before they look at a pointer.  Each
// returns 0 to go on, or the code to return, with a text in ddp_last_error() that begins with `who`, the entry's name.
// The shape: n_samples < 0, n <= 0, m < 0, 0 < rec_stride < 3 m, or an entry's own counts negative (counts_ok false).  per_sample: the
// receptor is one per sample (the joint minimiser): rec_stride >= 3 m, and not 0 when there is a receptor.
static inline int ddp_pose_check_shape(const char* who, int n_samples, int n, int m, int rec_stride, bool counts_ok, bool per_sample = false) {
  char msg[128];
  if (n_samples < 0 || n <= 0 || m < 0 || !counts_ok || (!per_sample && rec_stride != 0 && rec_stride < 3 * m)) {
    snprintf(msg, sizeof msg, "%s: shape", who);
    return ddp_fail(DDP_EINVAL, msg);
  }
  if (per_sample && (rec_stride < 3 * m || (m > 0 && rec_stride == 0))) {
    snprintf(msg, sizeof msg, "%s: rec is per sample, rec_stride >= 3 m", who);
    return ddp_fail(DDP_EINVAL, msg);
  }
  return 0;
}

// The ligand has to fit the kernel's LDS plan: n above the limit is DDP_ELIMIT, and the text names the limit's macro.
static inline int ddp_pose_check_atoms(const char* who, int n, int limit, const char* limit_name) {
  char msg[128];
  if (n <= limit) return 0;
  snprintf(msg, sizeof msg, "%s: more than %s ligand atoms", who, limit_name);
  return ddp_fail(DDP_ELIMIT, msg);
}
#define DDP_POSE_CHECK_ATOMS(who, n, LIMIT) ddp_pose_check_atoms(who, n, LIMIT, #LIMIT)

// The side-chain tables of the _flex entries (ddp_pose_minimize_flex, ddp_pose_search_flex, ddp_score_guidance_flex), counts already
// known not to be negative: the entry's limits on moving atoms and side-chain bonds and, where the entry has one (state_name not
// NULL), on the per-atom LDS state are DDP_ELIMIT and the text names the limit's macro; a table that its count needs and that is NULL
// is DDP_EINVAL.  (rec_anchor, upd_sc and the row state are the entries' own.)
static inline int ddp_pose_check_sidechains(const char* who, int n_mov, int n_sc, int n_sub, const void* mov, const void* sc_pairs,
                                            const void* sc_edge_idx, const void* sc_map, const void* sc_sub, int max_moving,
                                            const char* moving_name, int max_bonds, const char* bonds_name, size_t state, size_t max_state,
                                            const char* state_name) {
  char msg[160];
  if (n_mov > max_moving) snprintf(msg, sizeof msg, "%s: more than %s moving atoms", who, moving_name);
  else if (n_sc > max_bonds) snprintf(msg, sizeof msg, "%s: more than %s side-chain bonds", who, bonds_name);
  else if (state_name && state > max_state) snprintf(msg, sizeof msg, "%s: 89 n + 81 n_mov + 4 n_sc exceeds %s", who, state_name);
  else if ((n_mov > 0 && (!mov || !sc_pairs)) || (n_sc > 0 && (!sc_edge_idx || !sc_map)) || (n_sub > 0 && !sc_sub)) {
    snprintf(msg, sizeof msg, "%s: null argument", who);
    return ddp_fail(DDP_EINVAL, msg);
  } else return 0;
  return ddp_fail(DDP_ELIMIT, msg);
}
#define DDP_POSE_CHECK_SIDECHAINS(who, a, MOVING, BONDS, ...) \
  ddp_pose_check_sidechains(who, (a)->n_mov, (a)->n_sc, (a)->n_sub, (a)->mov, (a)->sc_pairs, (a)->sc_edge_idx, (a)->sc_map, (a)->sc_sub, MOVING, #MOVING, BONDS, #BONDS, __VA_ARGS__)

// The chain of the two search entries (a: ddp_search_args_t or ddp_search_flex_args_t), after the checks of the descent's pointers: the
// row state, the random numbers and the records (state_ok: what the entry's state holds beyond the shared pointers), then the descent's
// own scalars (descent_error: NULL, or what is wrong with them), then replicas, cycles, cycle0, temperature, step_init and the row count.
template <class Args>
static inline int ddp_pose_check_chain(const char* who, const Args* a, int n_samples, bool state_ok, const char* descent_error) {
  const char* what = nullptr;
  if (!a->perturb || !a->u || !a->cur_pos || !a->cur_e || !a->best_pos || !a->best_e || !a->best_cycle || !a->accepted || !a->trace || !a->flags ||
      !state_ok)
    what = "null perturb, u, state, trace or flags";
  else if (descent_error) what = descent_error;
  else if (a->replicas < 1 || a->cycles < 0 || a->cycle0 < 0) what = "replicas < 1, cycles or cycle0 < 0";
  else if (!(a->temperature > 0.0) || !isfinite(a->temperature)) what = "temperature must be positive and finite";
  else if (!(a->step_init > 0.0)) what = "step_init must be positive";
  else if ((int64_t)n_samples * a->replicas > 0x7fffffff) what = "n_samples * replicas does not fit a launch";
  if (!what) return 0;
  char msg[128];
  snprintf(msg, sizeof msg, "%s: %s", who, what);
  return ddp_fail(DDP_EINVAL, msg);
}

// After the launch: 0, or the launch's HIP error.
static inline int ddp_launch_result(const char* who) {
  const hipError_t err = hipGetLastError();
  if (err == hipSuccess) return 0;
  char where[96];
  snprintf(where, sizeof where, "%s launch", who);
  return ddp_fail_hip(err, where);
}

// Dynamic-LDS limit of a kernel, raised only when a launch needs more than any launch before it: hipFuncSetAttribute is not
// permitted while a stream is being captured (hipErrorStreamCaptureUnsupported), so a captured step must find the limit already
// set by the ordinary steps that ran before the capture (sampler.Sampler captures after two such steps).
static inline hipError_t ddp_need_lds(const void* kernel, int bytes, int* have) {
  if (bytes <= *have) return hipSuccess;
  const hipError_t err = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (err == hipSuccess) *have = bytes;
  return err;
}

// Occupancy shaping (ddp_set_occupancy_shaping, include/ddp_hip.h): launch-time LDS floors that decide how many workgroups of a kernel
// share a CU.  Plain ints read when a launch is enqueued.
extern int ddp_shape_rows_min_lds;      // ddp_conv_rows: dynamic LDS of a launch is at least this many bytes
extern int ddp_shape_stage_a_pad;       // ddp_stage_a*: dynamic LDS added to the kernels' static LDS

// Tiles per chunk of the conv launches' tile order (ddp_conv_deal of include/ddp_hip.h, resolved from the environment at the first call):
// what a launcher writes into ConvLaunch::deal_c
int ddp_conv_deal_chunk(void);

#endif
