// ddp_capi.hip - error bookkeeping and ABI version of libddp_hip.so.
#include <hip/hip_runtime.h>
#include <stdio.h>

#include <stddef.h>

#include "ddp_hip.h"
#include "ddp_internal.h"
#include "ddp_conv_deal.h"

// The layout of ABI version 17.  ddp_score_form_t sits in the four argument structs where their eleven doubles used to be spelled
// out: a caller compiled against the flat fields and this library agree on every byte.
static_assert(sizeof(ddp_score_form_t) == 88, "ddp_score_form_t: eleven doubles");
static_assert(sizeof(ddp_score_args_t) == 184 && offsetof(ddp_score_args_t, form) == 72, "ddp_score_args_t layout");
static_assert(sizeof(ddp_profile_args_t) == 192 && offsetof(ddp_profile_args_t, form) == 80, "ddp_profile_args_t layout");
static_assert(sizeof(ddp_minimize_args_t) == 272 && offsetof(ddp_minimize_args_t, form) == 104, "ddp_minimize_args_t layout");
static_assert(sizeof(ddp_minimize_flex_args_t) == 352 && offsetof(ddp_minimize_flex_args_t, form) == 104, "ddp_minimize_flex_args_t layout");

static thread_local char g_err[256] = "ok";

int ddp_fail(int code, const char* msg) {
  snprintf(g_err, sizeof(g_err), "%s", msg);
  return code;
}

int ddp_fail_hip(hipError_t err, const char* where) {
  snprintf(g_err, sizeof(g_err), "%s: %s", where, hipGetErrorString(err));
  return (int)err;
}

// DDP_CONV_DEAL in the environment (read at the first conv launch), or the value written here (tests, A/B tools): the tiles per chunk of
// the conv launches' chunk-cyclic tile order (ddp_deal_tile, csrc/ddp_conv_deal.h), 0 = one contiguous range of tiles per XCD.
// Results do not depend on it.
#define DDP_CONV_DEAL_DEFAULT 8
extern "C" int ddp_conv_deal;
int ddp_conv_deal = -1;
int ddp_conv_deal_chunk(void) {
  if (ddp_conv_deal < 0) {
    const char* e = getenv("DDP_CONV_DEAL");
    const int v = (e && e[0] >= '0' && e[0] <= '9') ? atoi(e) : DDP_CONV_DEAL_DEFAULT;
    ddp_conv_deal = (v > 4096) ? 4096 : v;
  }
  return (ddp_conv_deal > 4096) ? 4096 : ddp_conv_deal;
}
// the tile of workgroup `id` in a launch of `total` tiles dealt in chunks of c (the device's own function; tests/test_conv_deal_cpu.py)
extern "C" int ddp_conv_deal_tile(int id, int total, int c) {
  if (total < 1 || id < 0 || id >= total || c < 0 || c > 4096) {
    ddp_fail(DDP_EINVAL, "ddp_conv_deal_tile: id in [0, total), c in [0, 4096]");
    return -1;
  }
  return ddp_deal_tile(id, total, c);
}

int ddp_shape_rows_min_lds = 0;
int ddp_shape_stage_a_pad = 0;
// Launches enqueued after this call: ddp_conv_rows with at least `rows_min_lds_bytes` of dynamic LDS (> 80 KiB: ONE 4-wave workgroup per
// CU, i.e. one 256-register wave per SIMD, instead of two), the MFMA forms of ddp_stage_a* with `stage_a_lds_pad_bytes` on top of their
// static LDS (> 25 KiB: one workgroup per CU).  0 / 0 = the kernels' own occupancy.  Results do not depend on it.
extern "C" int ddp_set_occupancy_shaping(int rows_min_lds_bytes, int stage_a_lds_pad_bytes) {
  if (rows_min_lds_bytes < 0 || rows_min_lds_bytes > 160 * 1024 || stage_a_lds_pad_bytes < 0 || stage_a_lds_pad_bytes > 100 * 1024)
    return ddp_fail(DDP_EINVAL, "ddp_set_occupancy_shaping: bytes out of range");
  ddp_shape_rows_min_lds = rows_min_lds_bytes;
  ddp_shape_stage_a_pad = stage_a_lds_pad_bytes;
  return 0;
}

extern "C" int ddp_abi_version(void) { return DDP_ABI_VERSION; }
extern "C" const char* ddp_last_error(void) { return g_err; }

// 16 hex digits of the SHA-256 over the kernel sources this library was compiled from (diffdock_pocket_amd/build.py passes
// -DDDP_SRC_SHA16); _lib.load() compares it with the sources in the tree, so a stale binary cannot be loaded silently.
#ifndef DDP_SRC_SHA16
#define DDP_SRC_SHA16 "unknown"
#endif
// (the tag in front lets build.built_hash() find the hash in the file bytes without loading the library)
static const char ddp_src_tag[] = "DDP_SRC_SHA16=" DDP_SRC_SHA16;
extern "C" const char* ddp_source_hash(void) { return ddp_src_tag + 14; }
