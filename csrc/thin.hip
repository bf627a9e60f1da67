// Thinning a CSR corpus token by token: every token of a non-zero (document d, word w, count
// x) is kept with a probability p of its non-zero, and the kept / not kept tokens are
// compacted into two new CSRs on the device.
//
//   p      = rate                                              (constant-rate split), or
//          = theta[d, e] tw[e, w] / sum_k theta[d, k] tw[k, w]  (topic responsibility of
//            topic e: the HTM-WS submodel corpus), 0 where the denominator is 0, in [0, 1]
//   u_j    = u01(component j & 3 of rng4(seed, d, RNG_THIN | ((j >> 2) << 8), w))
//   kept   = sum_{j < x} [u_j < p]                             compared in fp32
//
// so kept is an exact Binomial(x, p) that depends on (seed, global document, word, token)
// alone: not on the grid, the chunking or the engine that makes the draws (the numpy twin
// of ops/thin.py makes the same ones).  Counts are integers in 0 .. 65535 (checked by the
// Python launcher), so the block index (j >> 2) < 2^14 never reaches the tag's low byte.
//
// Two passes, a wave per document, lanes over the row's non-zeros 64 at a time:
//
//   gfk_thin_count_k    p (the theta row in LDS x the topic-word matrix' column: K
//                       independent scattered loads per non-zero, summed in one fixed
//                       order), the draws, kept[e] into an int32 workspace, optionally
//                       p[e], and per row the number of non-zeros with kept > 0 and with
//                       x - kept > 0 (ballot + popcount)
//   (the launcher's caller turns the two count vectors into row offsets: a cumsum)
//   gfk_thin_compact_k  (index, kept) into the kept CSR and (index, x - kept) into the
//                       complement at out_ptr[d] + the lane's ballot prefix: column order
//                       is preserved and no zero is stored
//
// No atomics; the result is bitwise independent of grid and chunk.
#include "gfk_common.h"

using namespace gfk;

extern "C" {
typedef struct GfkThin {
  const int32_t *indptr, *indices;  // indptr: this chunk's row pointers (n_docs + 1)
  const float *values;
  const float *theta;      // [n_docs, K] rows of the chunk, or null: the constant rate
  const float *tw;         // [K, V] topic-word matrix, row stride ld (theta != null)
  int32_t *kept;           // workspace [nnz], addressed like indices / values
  float *p_out;            // optional [nnz]: the keep probabilities
  int32_t *n_kept, *n_rest;            // [n_docs] non-zeros of each output row (pass 1)
  const int32_t *kept_ptr, *rest_ptr;  // [n_docs] first output slot of each row (pass 2)
  int32_t *kept_idx;       // the kept CSR's indices / values
  float *kept_val;
  int32_t *rest_idx;       // the complement's (both null: not wanted)
  float *rest_val;
  uint64_t seed;
  float rate;
  int32_t n_docs, K, V, ld, topic;
  int32_t doc0;            // global index of the chunk's first document (RNG key)
  int32_t pass;            // 1: gfk_thin_count_k, 2: gfk_thin_compact_k
  int32_t max_grid;        // > 0: at most this many workgroups (tests: several rows per wave)
} GfkThin;
}

namespace {

constexpr int TH_THREADS = 256;
constexpr int TH_WAVES = TH_THREADS / 64;
constexpr int TH_MAX_K = 1024;      // theta row in LDS: 4 KiB per wave

// kept tokens of one non-zero: x draws in blocks of four, each compared with p in fp32.
// p <= 0 keeps nothing and p >= 1 everything (u < 1 always): no draw changes that.
__device__ __forceinline__ int thin_draw(uint64_t seed, uint32_t d, uint32_t w, int x, float p) {
  if (!(p > 0.f)) return 0;
  if (p >= 1.f) return x;
  int kept = 0;
  for (int j = 0; j < x; j += 4) {
    const uint4 r = rng4(seed, d, RNG_THIN | ((uint32_t)(j >> 2) << 8), w);
    kept += u01(r.x) < p;
    kept += (j + 1 < x) & (u01(r.y) < p);
    kept += (j + 2 < x) & (u01(r.z) < p);
    kept += (j + 3 < x) & (u01(r.w) < p);
  }
  return kept;
}

__global__ void __launch_bounds__(TH_THREADS) gfk_thin_count_k(GfkThin p) {
  __shared__ float ts[TH_WAVES][TH_MAX_K];
  const int lane = threadIdx.x & 63, wave = uniform(threadIdx.x >> 6);
  const int K = p.K, ld = p.ld, topic = p.topic;
  const bool by_topic = p.theta != nullptr;
  float* trow = ts[wave];
  for (int d = blockIdx.x * TH_WAVES + wave; d < p.n_docs; d += gridDim.x * TH_WAVES) {
    const int e0 = p.indptr[d], e1 = p.indptr[d + 1];
    if (by_topic) {
      for (int k = lane; k < K; k += 64) trow[k] = p.theta[(size_t)d * K + k];
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     // the wave's theta row is in LDS
      __builtin_amdgcn_wave_barrier();
    }
    const uint32_t dg = (uint32_t)(p.doc0 + d);
    int nk = 0, nr = 0;
    for (int eb = e0; eb < e1; eb += 64) {                   // (wave-uniform trip count)
      const int e = eb + lane;
      const bool on = e < e1;
      int x = 0, kept = 0;
      if (on) {
        const int w = p.indices[e];
        x = (int)p.values[e];
        float pr = p.rate;
        if (by_topic) {
          const float* bc = p.tw + w;
          float z0 = 0.f, z1 = 0.f;
          int k = 0;
#pragma unroll 4
          for (; k + 2 <= K; k += 2) {
            z0 += trow[k] * bc[(size_t)k * ld];
            z1 += trow[k + 1] * bc[(size_t)(k + 1) * ld];
          }
          if (k < K) z0 += trow[k] * bc[(size_t)k * ld];
          const float den = z0 + z1, num = trow[topic] * bc[(size_t)topic * ld];
          // num is one of den's terms: num >= den means every other term vanished
          pr = den > 0.f ? (num >= den ? 1.f : num / den) : 0.f;
          pr = fminf(fmaxf(pr, 0.f), 1.f);
        }
        kept = thin_draw(p.seed, dg, (uint32_t)w, x, pr);
        p.kept[e] = kept;
        if (p.p_out) p.p_out[e] = pr;
      }
      nk += __popcll(__ballot(on && kept > 0));
      nr += __popcll(__ballot(on && x - kept > 0));
    }
    if (lane == 0) {
      p.n_kept[d] = nk;
      if (p.n_rest) p.n_rest[d] = nr;
    }
    __builtin_amdgcn_wave_barrier();                         // (trow is rewritten for the next row)
  }
}

__global__ void __launch_bounds__(TH_THREADS) gfk_thin_compact_k(GfkThin p) {
  const int lane = threadIdx.x & 63, wave = uniform(threadIdx.x >> 6);
  const unsigned long long below = (1ull << lane) - 1ull;
  const bool want_rest = p.rest_idx != nullptr;
  for (int d = blockIdx.x * TH_WAVES + wave; d < p.n_docs; d += gridDim.x * TH_WAVES) {
    const int e0 = p.indptr[d], e1 = p.indptr[d + 1];
    int ok = p.kept_ptr[d], orr = want_rest ? p.rest_ptr[d] : 0;
    for (int eb = e0; eb < e1; eb += 64) {
      const int e = eb + lane;
      const bool on = e < e1;
      int w = 0, x = 0, kept = 0;
      if (on) {
        w = p.indices[e];
        x = (int)p.values[e];
        kept = p.kept[e];
      }
      const unsigned long long mk = __ballot(on && kept > 0);
      if (on && kept > 0) {
        const int o = ok + __popcll(mk & below);
        p.kept_idx[o] = w;
        p.kept_val[o] = (float)kept;
      }
      ok += __popcll(mk);
      if (want_rest) {
        const unsigned long long mr = __ballot(on && x - kept > 0);
        if (on && x - kept > 0) {
          const int o = orr + __popcll(mr & below);
          p.rest_idx[o] = w;
          p.rest_val[o] = (float)(x - kept);
        }
        orr += __popcll(mr);
      }
    }
  }
}

}  // namespace

extern "C" size_t gfk_thin_struct_size() { return sizeof(GfkThin); }

// the largest K of the topic responsibility mode
extern "C" int gfk_thin_max_topics() { return TH_MAX_K; }

// Host checks mirror the kernels' assumptions: a CSR with n_docs + 1 row pointers, the
// responsibility mode's 1 <= K <= gfk_thin_max_topics(), 0 <= topic < K, ld >= V; the
// complement either whole or absent.  Nothing is launched when a check fails.
extern "C" int gfk_thin(const GfkThin* p, hipStream_t s) {
  if (!p) return -7;
  if (p->n_docs < 0 || p->doc0 < 0 || p->V < 1) return -5;
  if ((p->pass != 1 && p->pass != 2) || p->max_grid < 0) return -5;
  if (!p->indptr || !p->indices || !p->values || !p->kept) return -7;
  const bool want_rest = p->rest_idx != nullptr;
  if ((p->rest_val != nullptr) != want_rest) return -7;
  if (p->pass == 1) {
    if (!p->n_kept) return -7;
    if (p->theta) {
      if (!p->tw) return -8;
      if (p->K < 1 || p->K > TH_MAX_K || p->topic < 0 || p->topic >= p->K || p->ld < p->V) return -5;
    } else if (!(p->rate >= 0.f && p->rate <= 1.f)) {
      return -5;
    }
  } else {
    if (!p->kept_ptr || !p->kept_idx || !p->kept_val) return -7;
    if (want_rest && !p->rest_ptr) return -7;
  }
  if (p->n_docs == 0) return 0;
  int grid = (p->n_docs + TH_WAVES - 1) / TH_WAVES;
  if (grid > 8192) grid = 8192;          // (the kernels stride over the documents)
  if (p->max_grid > 0 && grid > p->max_grid) grid = p->max_grid;
  if (p->pass == 1)
    hipLaunchKernelGGL(gfk_thin_count_k, dim3(grid), dim3(TH_THREADS), 0, s, *p);
  else
    hipLaunchKernelGGL(gfk_thin_compact_k, dim3(grid), dim3(TH_THREADS), 0, s, *p);
  return (int)hipGetLastError();
}
