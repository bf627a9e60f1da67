// Word co-occurrence counts of a corpus for topic coherence (NPMI):
//
//   counts[i][j] = #{ documents d : word_i and word_j both occur in d }      int64 [W, W]
//
// over a list of W vocabulary indices (the union of the topics' top words), straight from
// the device CSR.  A word occurs in a document when it has a stored entry with value > 0
// (stored zeros do not count); the diagonal is the document frequency.  Everything is an
// integer: no floats, no dense [D, W] operand, and sums that do not depend on their order,
// so neither the chunking of the documents nor the grid changes a single count, and counts
// of disjoint shards add up to the counts of their union.
//
// Two kernels per chunk of documents, after a memset of the bit matrix:
//
//   gfk_cooc_pack_k   one wave per group of 64 consecutive documents, lane = document.  Each
//                     lane walks its row, maps the word through slot[V] (position in the word
//                     list, -1 elsewhere) and ORs its bit into the slot's 64-bit mask in LDS
//                     (ds_or_b64; integer OR commutes).  The non-zero masks are stored as
//                     bits[slot][g], g = document / 64, so one slot's documents are one
//                     contiguous row of G = ceil(n_docs / 64) words.  Lanes past the last
//                     document set nothing.
//   gfk_cooc_count_k  counts[i][j] += sum_g popcount(bits[i][g] & bits[j][g]).  A work item is
//                     (pair of 64-slot tiles ti <= tj, range of g): W ~ 500 has 36 tile pairs
//                     for 256 CUs, so the document axis is split as well.  The two tiles'
//                     rows are staged through LDS 32 words of g at a time (row stride 33
//                     words: the 16 rows a wave reads at once fall on 16 distinct bank pairs);
//                     a thread keeps a 4 x 4 block of int32 partial counts (a launch covers
//                     fewer than 2^31 documents) and adds the non-zero ones to the int64
//                     matrix with integer global atomics, mirrored across the diagonal for
//                     ti < tj.  One AND + bit count covers 64 documents of a pair.
#include "gfk_common.h"

extern "C" {
typedef struct GfkCooc {
  const int32_t *indptr, *indices;  // indptr: this chunk's row pointers (n_docs + 1)
  const float *values;
  const int32_t *slot;              // [V]: position of a word in the word list, -1 elsewhere
  unsigned long long *bits;         // workspace [W, ceil(n_docs / 64)]
  long long *counts;                // [W, W], accumulated into (the caller zeroes it once)
  int64_t n_docs;                   // documents of this chunk
  int64_t bits_words;               // capacity of bits, in 64-bit words
  int32_t W, V;
  int32_t max_grid;                 // > 0: at most this many pack workgroups (tests); 0: below
} GfkCooc;
}

namespace {

constexpr int CO_MAX_W = 6144;     // 48 KiB of masks per wave (K = 512 topics x 10 words: 5120)
constexpr int CO_T = 64;           // slots per tile
constexpr int CO_GC = 32;          // words of g per staged chunk
constexpr int CO_LD = CO_GC + 1;   // LDS row stride (words)
constexpr int CO_THREADS = 256;
constexpr int CO_ITEMS = 2048;     // work items the count kernel aims for

typedef unsigned long long u64;

__global__ void __launch_bounds__(64) gfk_cooc_pack_k(GfkCooc p, int G) {
  extern __shared__ u64 co_mask[];
  const int lane = threadIdx.x, W = p.W;
  const int n_docs = (int)p.n_docs;
  for (int g = blockIdx.x; g < G; g += gridDim.x) {
    for (int s = lane; s < W; s += 64) co_mask[s] = 0;
    __syncthreads();
    const int d = g * 64 + lane;
    if (d < n_docs) {
      const int e1 = p.indptr[d + 1];
      for (int e = p.indptr[d]; e < e1; ++e) {
        const int v = p.indices[e];
        if (p.values[e] > 0.f && (unsigned)v < (unsigned)p.V) {
          const int s = p.slot[v];
          if ((unsigned)s < (unsigned)W) atomicOr(&co_mask[s], (u64)1 << lane);
        }
      }
    }
    __syncthreads();
    for (int s = lane; s < W; s += 64) {
      const u64 m = co_mask[s];
      if (m) p.bits[(size_t)s * G + g] = m;
    }
    __syncthreads();                         // the masks are cleared for the next group
  }
}

// stage rows [r0, r0 + 64) x words [gb, gb + 32) of bits; zero past W and past g1
__device__ inline void co_stage(u64* dst, const u64* bits, int r0, int W, int G, int gb, int g1) {
#pragma unroll
  for (int k = 0; k < CO_T * CO_GC / CO_THREADS; ++k) {
    const int idx = threadIdx.x + k * CO_THREADS;
    const int r = idx / CO_GC, c = idx % CO_GC;
    u64 v = 0;
    if (r0 + r < W && gb + c < g1) v = bits[(size_t)(r0 + r) * G + gb + c];
    dst[r * CO_LD + c] = v;
  }
}

__global__ void __launch_bounds__(CO_THREADS) gfk_cooc_count_k(GfkCooc p, int G, int nt, int gper) {
  __shared__ u64 ta[CO_T * CO_LD], tb[CO_T * CO_LD];
  int ti = 0, rem = blockIdx.x;              // blockIdx.x enumerates the pairs ti <= tj
  while (rem >= nt - ti) {
    rem -= nt - ti;
    ++ti;
  }
  const int tj = ti + rem, W = p.W;
  const int g0 = blockIdx.y * gper;
  const int g1 = g0 + gper < G ? g0 + gper : G;
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const u64* tbp = ti == tj ? ta : tb;
  int acc[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[r][c] = 0;
  for (int gb = g0; gb < g1; gb += CO_GC) {
    co_stage(ta, p.bits, ti * CO_T, W, G, gb, g1);
    if (ti != tj) co_stage(tb, p.bits, tj * CO_T, W, G, gb, g1);
    __syncthreads();
#pragma unroll 4
    for (int g = 0; g < CO_GC; ++g) {
      u64 a[4], b[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) a[r] = ta[(ty + 16 * r) * CO_LD + g];
#pragma unroll
      for (int c = 0; c < 4; ++c) b[c] = tbp[(tx + 16 * c) * CO_LD + g];
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] += __popcll(a[r] & b[c]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int i = ti * CO_T + ty + 16 * r, j = tj * CO_T + tx + 16 * c;
      if (i >= W || j >= W || acc[r][c] == 0) continue;
      atomicAdd((u64*)p.counts + (size_t)i * W + j, (u64)acc[r][c]);
      if (ti != tj) atomicAdd((u64*)p.counts + (size_t)j * W + i, (u64)acc[r][c]);
    }
}

}  // namespace

extern "C" size_t gfk_cooc_struct_size() { return sizeof(GfkCooc); }

// the largest word list the kernels take
extern "C" int gfk_cooc_max_words() { return CO_MAX_W; }

// Host checks mirror the kernels' assumptions: 1 <= W <= gfk_cooc_max_words(), a CSR with
// n_docs + 1 row pointers, n_docs in an int, a bit matrix of W * ceil(n_docs / 64) words.
// Nothing is launched when a check fails.
extern "C" int gfk_cooc(const GfkCooc* p, hipStream_t s) {
  if (!p) return -7;
  if (p->W < 1 || p->W > CO_MAX_W || p->V < 1 || p->max_grid < 0) return -5;
  if (p->n_docs < 0 || p->n_docs >= ((int64_t)1 << 31) - 64) return -6;
  if (!p->indptr || !p->indices || !p->values || !p->slot || !p->bits || !p->counts) return -7;
  if (p->n_docs == 0) return 0;
  const int G = (int)((p->n_docs + 63) / 64);
  if (p->bits_words < (int64_t)p->W * G) return -9;
  hipError_t e = hipMemsetAsync(p->bits, 0, sizeof(u64) * (size_t)p->W * G, s);
  if (e != hipSuccess) return (int)e;
  const size_t smem = sizeof(u64) * (size_t)p->W;
  e = hipFuncSetAttribute((const void*)gfk_cooc_pack_k, hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)smem);
  if (e != hipSuccess) return (int)e;
  int pgrid = G < 4096 ? G : 4096;           // (the kernel strides over the groups)
  if (p->max_grid > 0 && pgrid > p->max_grid) pgrid = p->max_grid;
  hipLaunchKernelGGL(gfk_cooc_pack_k, dim3(pgrid), dim3(64), smem, s, *p, G);
  int rc = (int)hipGetLastError();
  if (rc) return rc;
  // the split of the document axis only sizes the grid: integer sums do not depend on it
  const int nt = (p->W + CO_T - 1) / CO_T;
  const int npair = nt * (nt + 1) / 2;
  const int nchunk = (G + CO_GC - 1) / CO_GC;
  int nsplit = (CO_ITEMS + npair - 1) / npair;
  if (nsplit > nchunk) nsplit = nchunk;
  const int gper = (nchunk + nsplit - 1) / nsplit * CO_GC;
  nsplit = (G + gper - 1) / gper;
  hipLaunchKernelGGL(gfk_cooc_count_k, dim3(npair, nsplit), dim3(CO_THREADS), 0, s, *p, G, nt, gper);
  return (int)hipGetLastError();
}
