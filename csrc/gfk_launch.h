// Host side of the fused-step kernel families: one launch path and one instance table.
//
// Every model kernel exists in two argument forms (gfk_common.h GfkArgT): <false> takes the
// descriptor by value for one client, <true> a pointer to the device array with grid z =
// the clients.  A GfkKernel names a kernel in both forms; gfk_launch picks the form from
// m->n_batch.  A family lists its instances ONCE, as a static table of {key, kernel} rows:
// the launcher looks its instance up by the runtime values it dispatches on (gfk_find), and
// the family's *_set_smem raises the dynamic-LDS limit of the same rows (gfk_raise_lds) --
// so an instance a launcher can reach is an instance gfk_setup covers, and a new instance
// is one new row.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "gfk_common.h"

// A kernel in both argument forms; either may be null (batched-only / one-client-only
// kernels), and launching the missing form is an error.
template <template <bool> class... A>
struct GfkKernelT {
  void (*one)(A<false>...);
  void (*many)(A<true>...);
};
typedef GfkKernelT<GfkArgT> GfkKernel;             // kernel(GfkArgT)
typedef GfkKernelT<GfkArgT, GfkUArgT> GfkKernelU;  // kernel(GfkArgT, GfkUArgT): the W_in update's

// {one-client, batched} of a kernel template whose LAST parameter is the batched flag
#define GFK_PAIR(name, ...) {name<__VA_ARGS__, false>, name<__VA_ARGS__, true>}

// One row of a family's instance table: up to four key values (unused ones 0) and the kernel.
template <class K>
struct GfkRowT {
  int key[4];
  K k;
};
typedef GfkRowT<GfkKernel> GfkRow;
typedef GfkRowT<GfkKernelU> GfkRowU;

// the row with exactly this key, or null
template <class K, size_t N>
__host__ inline const K* gfk_find(const GfkRowT<K> (&t)[N], int a, int b = 0, int c = 0, int d = 0) {
  for (const GfkRowT<K>& r : t)
    if (r.key[0] == a && r.key[1] == b && r.key[2] == c && r.key[3] == d) return &r.k;
  return nullptr;
}

// Raise every instance of the table to `bytes` of dynamic LDS.  (Plan time only -- gfk_setup:
// a kernel's first launch may already be inside a graph capture.)
template <class K, size_t N>
__host__ inline int gfk_raise_lds(const GfkRowT<K> (&t)[N], size_t bytes) {
  for (const GfkRowT<K>& r : t)
    for (const void* f : {(const void*)r.k.one, (const void*)r.k.many}) {
      if (!f) continue;
      hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
      if (e != hipSuccess) return (int)e;
    }
  return 0;
}

// The attribute is per function and process-wide: a family only ever raises it, so an engine
// built earlier with a larger footprint keeps launching after a smaller one is set up.
// `cur` is the family's high-water mark.
__host__ inline bool gfk_lds_raised(size_t& cur, size_t bytes) {
  if (bytes <= cur) return false;
  cur = bytes;
  return true;
}

__host__ inline int gfk_launch_form(const void* f, dim3 g, dim3 b, void** args, size_t sm, hipStream_t s) {
  if (!f) return -1;                    // the kernel has no such form
  (void)hipLaunchKernel(f, g, b, args, sm, s);
  return (int)hipGetLastError();
}

// Launch k (null: no instance for the key, -1) for m: one client with grid g and the
// descriptor by value, or the batched form with grid z = the clients and the device array.
// (GfkArgT<false> / GfkUArgT<false> hold exactly the descriptor: the host's copy is the argument.)
static_assert(sizeof(GfkArgT<false>) == sizeof(GfkModel) && sizeof(GfkUArgT<false>) == sizeof(GfkUpdate), "");
__host__ inline int gfk_launch(const GfkKernel* k, const GfkModel* m, dim3 g, dim3 b, size_t sm, hipStream_t s) {
  if (!k) return -1;
  if (m->n_batch > 1) {
    const GfkModel* p = gfk_dev(m);
    void* args[] = {&p};
    return gfk_launch_form((const void*)k->many, gfk_grid(g, m), b, args, sm, s);
  }
  void* args[] = {const_cast<GfkModel*>(m)};
  return gfk_launch_form((const void*)k->one, g, b, args, sm, s);
}
__host__ inline int gfk_launch(const GfkKernelU* k, const GfkModel* m, const GfkUpdate* u, dim3 g, dim3 b,
                               size_t sm, hipStream_t s) {
  if (!k) return -1;
  if (m->n_batch > 1) {
    const GfkModel* p = gfk_dev(m);
    const GfkUpdate* pu = reinterpret_cast<const GfkUpdate*>(m->dev_upd);
    void* args[] = {&p, &pu};
    return gfk_launch_form((const void*)k->many, gfk_grid(g, m), b, args, sm, s);
  }
  void* args[] = {const_cast<GfkModel*>(m), const_cast<GfkUpdate*>(u)};
  return gfk_launch_form((const void*)k->one, g, b, args, sm, s);
}
