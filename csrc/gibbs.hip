// Collapsed Gibbs sampling for LDA in the form Mallet's ParallelTopicModel runs it: the
// document-topic counts are live, the word-topic counts are frozen for a sweep, and the
// "threads" are documents -- a wave per document.
//
// State (ops/lda.py): the tokens of document d in storage order of its CSR row, a non-zero
// (w, x) being x consecutive tokens; tok_ptr[e] the exclusive cumsum of the counts (N < 2^31
// tokens); z[N] uint16 assignments; nwk[V, K], nk[K], ndk[D, K] int32.
//
//   u(i)   = u01(component i & 3 of rng4(seed, sweep, RNG_GIBBS | ((i >> 2) << 8), g))
//            token i of global document g; sweep 0 is the initialisation, sweeps count from 1
//   init   z = min(K - 1, floor(u K))                                      in fp32
//   sweep  for every token in order, old topic o, word w:
//            ndk[o] -= 1
//            p_k   = (ndk[k] + alpha_k) (nwk0[w][k] - [k = o] + beta) / (nk0[k] - [k = o] + V beta)
//            cum   = inclusive prefix sum of p over k, target = u cum[K - 1]
//            k'    = min(K - 1, #{k : cum_k <= target});  z = k';  ndk[k'] += 1
//          nwk0 / nk0 are the counts at the start of the sweep; `frozen` (fold-in of unseen
//          documents) drops the [k = o] terms: the counts are somebody else's
//   recount  nwk from z, integers only: an inverted index of the non-zeros by word, a work
//          item = (word, at most `seg` of its non-zeros), an LDS histogram per item; a word of
//          one item writes its row, a split word's items write partial rows that the merge
//          pass sums (integer sums: every split gives the same counts)
//
// The sweep: lane l owns the T = ceil(K / 64) topics l T .. l T + T - 1, their ndk in
// registers (rebuilt per document from z by an integer LDS histogram in the wave's slice).
// A token costs T products, a DPP prefix sum over the lanes' totals (row_shr 1 2 4 8, then
// row_bcast 15 / 31), T ballots.  The word's nwk0 row is loaded once per non-zero, the next
// non-zero's row while the current one is sampled.  Draws and old assignments are fetched
// 64 tokens at a time, new assignments stored 64 at a time.
//
// No atomics on global memory, no float atomics anywhere; every loop is bounded; the result
// is bitwise independent of grid, chunking and max_grid.
#include "gfk_common.h"

using namespace gfk;

extern "C" {
typedef struct GfkLda {
  const int32_t* indptr;     // this chunk's row pointers (n_docs + 1), offsets into indices
  const int32_t* indices;    // [nnz] words
  const int32_t* tok_ptr;    // [nnz + 1] first token of every non-zero
  uint16_t* z;               // [N]
  const int32_t* nwk0;       // [V, K] counts at the start of the sweep
  const int32_t* nk0;        // [K]
  const float* alpha;        // [K]
  int32_t* ndk;              // optional [n_docs, K] rows of the chunk: the final counts
  const int32_t* inv;        // recount: non-zero ids sorted by word (stable)
  const int32_t *item_lo, *item_hi;   // [n_items] the item's range of inv
  const int32_t* item_row;   // [n_items] r >= 0: row r of nwk; r < 0: row -1 - r of part
  const int32_t *mrg_word, *mrg_first, *mrg_n;   // merge [n_items]: nwk[word] = sum of n part rows
  int32_t* nwk;              // recount / merge: the rows written
  int32_t* part;             // partial rows of the split words
  uint64_t seed;
  float beta, vbeta;         // beta, V beta
  int32_t n_docs, n_items, K, V;
  int32_t doc0;              // global index of the chunk's first document (RNG key)
  int32_t sweep;             // Philox step: 0 init, >= 1 sweeps
  int32_t frozen;            // sweep: no own-token exclusion
  int32_t pass;              // 1 init, 2 sweep, 3 recount, 4 merge
  int32_t max_grid;          // > 0: at most this many workgroups
} GfkLda;
}

namespace {

constexpr int LDA_THREADS = 256;
constexpr int LDA_WAVES = LDA_THREADS / 64;
constexpr int LDA_MAX_K = 512;
constexpr int LDA_MAX_DOC_TOKENS = 1 << 26;     // (i >> 2) << 8 stays in 32 bits

__device__ __forceinline__ float lda_u(uint64_t seed, uint32_t sweep, uint32_t g, int i) {
  const uint4 r = rng4(seed, sweep, RNG_GIBBS | ((uint32_t)(i >> 2) << 8), g);
  const int c = i & 3;
  return u01(c == 0 ? r.x : c == 1 ? r.y : c == 2 ? r.z : r.w);
}

__device__ __forceinline__ int lane_i(int v, int l) { return __builtin_amdgcn_readlane(v, l); }
__device__ __forceinline__ float lane_f(float v, int l) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}
__device__ __forceinline__ void lds_sync() {      // the wave's own LDS traffic, in order
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}

// DPP with row / bank masks: lanes outside the masks, and lanes whose source falls outside
// the row, keep 0 (the sum's identity).
template <int CTRL, int ROWS>
__device__ __forceinline__ float dpp0(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, ROWS, 0xF, false));
}
// Inclusive prefix sum over the 64 lanes: Kogge-Stone inside each row of 16 (row_shr 1, 2, 4,
// 8), then lane 15 of rows 0 / 2 into rows 1 / 3 (row_bcast15) and lane 31 into rows 2, 3
// (row_bcast31).
__device__ __forceinline__ float wave_scan(float v) {
  v += dpp0<0x111, 0xF>(v);
  v += dpp0<0x112, 0xF>(v);
  v += dpp0<0x114, 0xF>(v);
  v += dpp0<0x118, 0xF>(v);
  v += dpp0<0x142, 0xA>(v);
  v += dpp0<0x143, 0xC>(v);
  return v;
}
// lane l receives lane l - 1's value, lane 0 receives 0 (wave_shr 1)
__device__ __forceinline__ float wave_shr1(float v) { return dpp0<0x138, 0xF>(v); }

__global__ void __launch_bounds__(LDA_THREADS) gfk_lda_init_k(GfkLda p) {
  const int lane = threadIdx.x & 63, wave = uniform(threadIdx.x >> 6);
  const int K = p.K;
  const float fk = (float)K;
  for (int d = blockIdx.x * LDA_WAVES + wave; d < p.n_docs; d += gridDim.x * LDA_WAVES) {
    const int e0 = p.indptr[d], e1 = p.indptr[d + 1];
    const int t0 = p.tok_ptr[e0], n = p.tok_ptr[e1] - t0;
    const uint32_t g = (uint32_t)(p.doc0 + d);
    for (int i = lane; i < n; i += 64) {
      const int k = (int)floorf(lda_u(p.seed, 0u, g, i) * fk);
      p.z[(size_t)t0 + i] = (uint16_t)min(K - 1, k);
    }
  }
}

template <int T>
__device__ __forceinline__ void lda_row(int (&nw)[T], const int32_t* nwk0, int w, int K, int k0) {
  const int32_t* row = nwk0 + (size_t)w * K;
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const int v = row[min(k0 + t, K - 1)];
    nw[t] = k0 + t < K ? v : 0;
  }
}

template <int T>
__global__ void __launch_bounds__(LDA_THREADS) gfk_lda_sweep_k(GfkLda p) {
  __shared__ int hist[LDA_WAVES][LDA_MAX_K];
  const int lane = threadIdx.x & 63, wave = uniform(threadIdx.x >> 6);
  const int K = p.K, k0 = lane * T;
  const bool frozen = p.frozen != 0;
  const float beta = p.beta, vbeta = p.vbeta;
  int* h = hist[wave];
  // the lane's topics: alpha, 1 / (nk0 + V beta) and 1 / (nk0 - 1 + V beta); a topic past K
  // gets alpha = 0 and a zero factor, so its p is an exact 0
  float al[T], rd[T], rdo[T];
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const int k = min(k0 + t, K - 1);
    const bool on = k0 + t < K;
    const int nk = p.nk0[k];
    al[t] = on ? p.alpha[k] : 0.f;
    rd[t] = on ? __builtin_amdgcn_rcpf((float)nk + vbeta) : 0.f;
    rdo[t] = on ? __builtin_amdgcn_rcpf((float)(nk - 1) + vbeta) : 0.f;
  }
  for (int d = blockIdx.x * LDA_WAVES + wave; d < p.n_docs; d += gridDim.x * LDA_WAVES) {
    const int e0 = p.indptr[d], e1 = p.indptr[d + 1];
    const int t0 = p.tok_ptr[e0], n = p.tok_ptr[e1] - t0;
    const uint32_t g = (uint32_t)(p.doc0 + d);
    uint16_t* zd = p.z + (size_t)t0;
    // ---- the document's ndk from z: an integer histogram in the wave's LDS slice
    for (int k = lane; k < T * 64; k += 64) h[k] = 0;
    lds_sync();
    for (int i = lane; i < n; i += 64) atomicAdd(&h[min((int)zd[i], K - 1)], 1);
    lds_sync();
    int nd[T];
#pragma unroll
    for (int t = 0; t < T; ++t) nd[t] = h[k0 + t];
    lds_sync();                                   // (h is zeroed again for the next document)
    // ---- the tokens in order
    int i = 0;                                    // token of the document (wave-uniform)
    int zl = 0, zn = 0;                           // lane s: old / new topic of token (i & ~63) + s
    float ul = 0.f;                               //         its draw
    for (int eb = e0; eb < e1; eb += 64) {
      const int e = min(eb + lane, e1 - 1);
      const int wl = p.indices[e];
      const int xl = p.tok_ptr[e + 1] - p.tok_ptr[e];
      const int cnt = min(64, e1 - eb);
      int nw[T], nx[T];
      lda_row<T>(nw, p.nwk0, lane_i(wl, 0), K, k0);
      for (int j = 0; j < cnt; ++j) {
        const int x = lane_i(xl, j);
        lda_row<T>(nx, p.nwk0, lane_i(wl, min(j + 1, cnt - 1)), K, k0);   // the next row, early
        for (int tt = 0; tt < x && i < n; ++tt, ++i) {
          const int s = i & 63;
          if (s == 0) {                           // the next 64 tokens' topics and draws
            const int ii = i + lane;
            zl = ii < n ? (int)zd[ii] : 0;
            zn = zl;
            ul = lda_u(p.seed, (uint32_t)p.sweep, g, ii);
          }
          const int o = min(lane_i(zl, s), K - 1);
          const float u = lane_f(ul, s);
          float c[T], run = 0.f;
#pragma unroll
          for (int t = 0; t < T; ++t) {
            const bool io = k0 + t == o;
            nd[t] -= io;
            const bool ex = io && !frozen;
            const float a = (float)nd[t] + al[t];
            const float b = (float)(nw[t] - (int)ex) + beta;
            run += a * b * (ex ? rdo[t] : rd[t]);
            c[t] = run;
          }
          const float below = wave_shr1(wave_scan(run));     // sum over the lanes before this one
          const float total = lane_f(below + c[T - 1], 63);  // cum[K - 1]: the rest adds zeros
          const float target = u * total;
          int kn = 0;
#pragma unroll
          for (int t = 0; t < T; ++t)
            kn += __popcll(__ballot(k0 + t < K && below + c[t] <= target));
          kn = min(kn, K - 1);
#pragma unroll
          for (int t = 0; t < T; ++t) nd[t] += k0 + t == kn;
          if (lane == s) zn = kn;
          if (s == 63 || i == n - 1) {
            const int ii = i - s + lane;
            if (lane <= s && ii < n) zd[ii] = (uint16_t)zn;
          }
        }
#pragma unroll
        for (int t = 0; t < T; ++t) nw[t] = nx[t];
      }
    }
    if (p.ndk) {
#pragma unroll
      for (int t = 0; t < T; ++t)
        if (k0 + t < K) p.ndk[(size_t)d * K + k0 + t] = nd[t];
    }
  }
}

__global__ void __launch_bounds__(LDA_THREADS) gfk_lda_recount_k(GfkLda p) {
  __shared__ int hist[LDA_WAVES][LDA_MAX_K];
  const int lane = threadIdx.x & 63, wave = uniform(threadIdx.x >> 6);
  const int K = p.K;
  int* h = hist[wave];
  for (int it = blockIdx.x * LDA_WAVES + wave; it < p.n_items; it += gridDim.x * LDA_WAVES) {
    for (int k = lane; k < K; k += 64) h[k] = 0;
    lds_sync();
    const int lo = p.item_lo[it], hi = p.item_hi[it];
    for (int b = lo; b < hi; b += 64) {
      if (b + lane < hi) {
        const int e = p.inv[b + lane];
        const int ta = p.tok_ptr[e], tb = p.tok_ptr[e + 1];
        for (int t = ta; t < tb; ++t) atomicAdd(&h[min((int)p.z[t], K - 1)], 1);
      }
    }
    lds_sync();
    const int r = p.item_row[it];
    int32_t* dst = r >= 0 ? p.nwk + (size_t)r * K : p.part + (size_t)(-1 - r) * K;
    for (int k = lane; k < K; k += 64) dst[k] = h[k];
    lds_sync();
  }
}

__global__ void __launch_bounds__(LDA_THREADS) gfk_lda_merge_k(GfkLda p) {
  const int lane = threadIdx.x & 63, wave = uniform(threadIdx.x >> 6);
  const int K = p.K;
  for (int m = blockIdx.x * LDA_WAVES + wave; m < p.n_items; m += gridDim.x * LDA_WAVES) {
    const int w = p.mrg_word[m], f = p.mrg_first[m], c = p.mrg_n[m];
    for (int k = lane; k < K; k += 64) {
      int s = 0;
      for (int j = 0; j < c; ++j) s += p.part[(size_t)(f + j) * K + k];
      p.nwk[(size_t)w * K + k] = s;
    }
  }
}

template <int T>
void lda_sweep_launch(const GfkLda* p, int grid, hipStream_t s) {
  hipLaunchKernelGGL(gfk_lda_sweep_k<T>, dim3(grid), dim3(LDA_THREADS), 0, s, *p);
}

}  // namespace

extern "C" size_t gfk_lda_struct_size() { return sizeof(GfkLda); }
extern "C" int gfk_lda_max_topics() { return LDA_MAX_K; }
extern "C" int gfk_lda_max_doc_tokens() { return LDA_MAX_DOC_TOKENS; }

// Host checks mirror the kernels' assumptions; the launcher (ops/lda.py) has checked the CSR,
// the counts, the token totals and the item tables.  Nothing is launched when a check fails.
extern "C" int gfk_lda(const GfkLda* p, hipStream_t s) {
  if (!p) return -7;
  if (p->pass < 1 || p->pass > 4 || p->max_grid < 0) return -5;
  if (p->K < 1 || p->K > LDA_MAX_K || p->V < 1) return -5;
  if (!p->tok_ptr || !p->z) return -7;
  int work;
  if (p->pass <= 2) {
    if (p->n_docs < 0 || p->doc0 < 0 || p->sweep < 0) return -5;
    if (!p->indptr || !p->indices) return -7;
    if (p->pass == 1 && p->sweep != 0) return -5;
    if (p->pass == 2) {
      if (p->sweep < 1 || !(p->beta > 0.f) || !(p->vbeta > 0.f)) return -5;
      if (!p->nwk0 || !p->nk0 || !p->alpha) return -7;
    }
    work = p->n_docs;
  } else {
    if (p->n_items < 0) return -5;
    if (!p->nwk) return -7;
    if (p->pass == 3 && (!p->inv || !p->item_lo || !p->item_hi || !p->item_row)) return -7;
    if (p->pass == 4 && (!p->mrg_word || !p->mrg_first || !p->mrg_n || !p->part)) return -7;
    work = p->n_items;
  }
  if (work == 0) return 0;
  int grid = (work + LDA_WAVES - 1) / LDA_WAVES;
  if (grid > 16384) grid = 16384;          // (the kernels stride over their work)
  if (p->max_grid > 0 && grid > p->max_grid) grid = p->max_grid;
  switch (p->pass) {
    case 1: hipLaunchKernelGGL(gfk_lda_init_k, dim3(grid), dim3(LDA_THREADS), 0, s, *p); break;
    case 2:
      switch ((p->K + 63) / 64) {
        case 1: lda_sweep_launch<1>(p, grid, s); break;
        case 2: lda_sweep_launch<2>(p, grid, s); break;
        case 3: lda_sweep_launch<3>(p, grid, s); break;
        case 4: lda_sweep_launch<4>(p, grid, s); break;
        case 5: lda_sweep_launch<5>(p, grid, s); break;
        case 6: lda_sweep_launch<6>(p, grid, s); break;
        case 7: lda_sweep_launch<7>(p, grid, s); break;
        default: lda_sweep_launch<8>(p, grid, s); break;
      }
      break;
    case 3: hipLaunchKernelGGL(gfk_lda_recount_k, dim3(grid), dim3(LDA_THREADS), 0, s, *p); break;
    default: hipLaunchKernelGGL(gfk_lda_merge_k, dim3(grid), dim3(LDA_THREADS), 0, s, *p); break;
  }
  return (int)hipGetLastError();
}
