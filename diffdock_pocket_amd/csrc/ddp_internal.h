// ddp_internal.h - shared helpers of libddp_hip.so (not part of the C ABI).
#ifndef DDP_INTERNAL_H
#define DDP_INTERNAL_H
#include <hip/hip_runtime.h>
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
