// ddp_pockets_uf.h - the lock-free union-find of ddp_pocket_label (ddp_pockets.hip), as host + device code so that the same helpers
// run in a stand-alone host program under the host sanitizers (tools/pocket_uf_check.cpp) before they run on a GPU.
//
// parent[i] is -1 outside the mask, else an index of i's component with parent[i] <= i; a root has parent[i] == i.  The only writes
// after the initialisation are uf_min(&parent[a], b) with b < a, so a parent only ever decreases.  Termination:
//   uf_find  walks a strictly decreasing chain of non-negative indices: at most n steps, whatever other threads write meanwhile
//            (a value read late or early is still a smaller index of the same component).
//   uf_union each retry continues with a pair whose larger member is strictly smaller than before (see the loop): at most n retries.
// Nothing waits for another thread, so there is no livelock.  A root is the smallest index of its tree; when every edge has been
// united, a component is one tree, and its root is the component's smallest flat index - independent of the order of the atomics.
#ifndef DDP_POCKETS_UF_H
#define DDP_POCKETS_UF_H
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define DDP_UF_HD __host__ __device__ __forceinline__
#else
#define DDP_UF_HD inline
#endif

DDP_UF_HD int32_t uf_load(const int32_t* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // past the CU's L1: other workgroups lower parents
#else
  return __atomic_load_n(p, __ATOMIC_RELAXED);
#endif
}

// *p = min(*p, v) atomically; returns the value before
DDP_UF_HD int32_t uf_min(int32_t* p, int32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return atomicMin(p, v);
#else
  int32_t old = __atomic_load_n(p, __ATOMIC_RELAXED);
  while (old > v && !__atomic_compare_exchange_n(p, &old, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {
  }   // (a failed exchange reloads `old`, which another thread has lowered: finite)
  return old;
#endif
}

DDP_UF_HD int32_t uf_find(const int32_t* parent, int32_t i) {
  for (;;) {
    const int32_t p = uf_load(parent + i);
    if (p == i) return i;
    i = p;   // p < i
  }
}

DDP_UF_HD void uf_union(int32_t* parent, int32_t a, int32_t b) {
  for (;;) {
    a = uf_find(parent, a);
    b = uf_find(parent, b);
    if (a == b) return;
    if (a < b) {
      const int32_t t = a;
      a = b;
      b = t;
    }
    // a > b: hang a below b if a is still a root
    const int32_t old = uf_min(parent + a, b);
    if (old == a) return;
    // a had been hung below old < a by another thread meanwhile; parent[a] is now min(old, b), and what remains is to unite old with
    // b: both are smaller than a, so the larger member of the pair has decreased
    a = old;
  }
}

#endif
