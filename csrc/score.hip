// Held-out scoring: the per-document ELBO terms of a whole corpus on the eval-mode
// ProdLDA decoder (reference avitm.py:295-321 _validation, decoder_network.py:109-135 in
// eval mode, avitm.py:207-225 the loss terms).
//
//   theta[r]  = softmax(mu_d + eps_{d,s} sigma_d)          row r = (document d, draw s)
//   zn[r, v]  = (sum_k theta[r, k] beta[k, v] - beta_rm[v]) rsqrt(beta_rv[v] + bn_eps)
//   lse[r]    = log sum_{v < V} exp(zn[r, v])
//   RL[r]     = - sum_{v in nz(d)} x_v log(exp(zn[r, v] - lse[r]) + 1e-10)
//   KL[d]     = the closed-form Gaussian KL of the posterior moments against the prior
//
// Four launches per chunk of documents, after gfk_theta_infer has left the posterior
// moments (the encoder runs once per document):
//
//   gfk_score_theta_k  one wave per document: KL[d], and the draws' theta rows -- the
//                      normals of csrc/infer.hip (RNG_INFER, keyed by seed, global document
//                      index, topic; draw s is element s % 4 of counter s / 4), so a row
//                      does not depend on the grid or the chunking; n_samples = 0 is the
//                      plug-in theta = softmax(mu), no RNG
//   gfk_doc_score_k    the decoder's log-sum-exp: a persistent workgroup (4 waves) takes
//                      work items (block of 64 rows -- 32 above K = 256 --, vocabulary
//                      range), stages the block's theta once and streams beta over ALL vocab
//                      tiles of 64 columns of the range in chunks of 32 topics, so the LDS
//                      use does not grow with K beyond the theta block.  A large vocabulary
//                      is cut into up to 8 ranges (a function of V alone): a workgroup
//                      streams beta at a few GB/s (256-byte row segments), so a validation
//                      set of a few thousand rows needs the ranges to occupy the CUs.  Wave w
//                      owns the tile's columns 16 w .. 16 w + 15 for every row tile; the
//                      fp32 MFMA accumulators feed the running-statistics batch-norm and a
//                      per-lane ONLINE (max, sum) pair per row -- with running statistics
//                      the logits are unbounded (the training forward's are not: its batch
//                      statistics bound |z| <= sqrt(nb - 1)), so the sum-exp is max-shifted.
//                      After the range's last tile the row's (max, sum) pairs are merged in a
//                      fixed order into one partial per (range, row).
//   gfk_score_sparse_k one wave per row: lse = the ranges' partials merged in range order;
//                      the logits of the row's non-zeros alone are recomputed (theta row in
//                      LDS x beta's column) and lse and the +1e-10 applied.  No [rows, V]
//                      array exists anywhere.
//   gfk_score_mean_k   RL[d] = mean over the draws' rows, in draw order.
//
// Always fp32 (scoring is a measurement), no atomics, fixed-order reductions.
#include "gfk_common.h"

using namespace gfk;

extern "C" {
typedef struct GfkScore {
  const int32_t *indptr, *indices;  // indptr: this chunk's row pointers (n_docs + 1)
  const float *values;
  const float *moments;  // [n_docs, 2, K] posterior (mu | log-sigma^2) of the chunk (gfk_theta_infer)
  float *theta;          // workspace [n_docs * R, K], R = max(n_samples, 1) rows per document
  float *lse_part;       // workspace [gfk_score_vranges(V), n_docs * R, 2]: (max, sum exp) partials
  float *rl_rows;        // workspace [n_docs * R]
  float *out;            // [n_docs, 2] = (KL, RL)
  int32_t n_docs, n_samples;
  uint64_t seed;
  int32_t grid, doc0;    // doc0: global index of the chunk's first document (RNG key)
  int32_t max_grid;      // > 0: no launch but gfk_score_mean_k gets more workgroups (tests: the
                         // strided loops take several work items each); 0: the grids below
} GfkScore;
}

namespace {

constexpr int SC_THREADS = 256;
constexpr int SC_WAVES = SC_THREADS / 64;
constexpr int SC_VB = 64;      // vocab tile
constexpr int SC_KC = 32;      // beta rows (topics) per staged chunk
constexpr int SC_LDB = 80;     // chunk row stride: B-role reads (4 k x 16 columns) conflict free
constexpr int SC_BU = SC_KC * SC_VB / SC_THREADS;   // chunk elements per thread
constexpr int SC_KQ = 8;       // topics per lane of the theta kernel (K <= 512)

// the decoder's view of the model
struct ScoreArgs {
  const float *beta, *beta_rm, *beta_rv, *prior_mean, *prior_var;
  int V, K, ldb;
  float bn_eps;
};

__host__ __device__ inline int sc_kp(int K) { return (K + 3) & ~3; }
// theta block row stride: 2 x odd, so the A-role reads (16 rows x 2 k per half-wave) land
// on 32 distinct banks, and >= K padded to whole MFMA k-steps (zero padding)
__host__ __device__ inline int sc_kts(int K) { return sc_kp(K) + 2; }
__host__ __device__ inline int sc_row_tiles(int K) { return K <= 256 ? 4 : 2; }
// vocabulary ranges a row block is split into (one work item each): a function of V alone,
// so the merge order of a row's partials -- the result's bits -- depends on neither the
// grid nor the chunking.  One range per 64 tiles, at most 8.
__host__ __device__ inline int sc_vranges(int V) {
  const int r = (V + SC_VB - 1) / SC_VB / 64;
  return r < 1 ? 1 : (r > 8 ? 8 : r);
}
__host__ __device__ inline size_t sc_smem_floats(int K) {
  const int BR = 16 * sc_row_tiles(K);
  return (size_t)BR * sc_kts(K) + SC_KC * SC_LDB + SC_WAVES * BR * 2;
}

__global__ void __launch_bounds__(SC_THREADS) gfk_score_theta_k(ScoreArgs a, GfkScore p) {
  const int lane = threadIdx.x & 63, wave = uniform(threadIdx.x >> 6);
  const int K = a.K, S = p.n_samples, R = S > 0 ? S : 1;
  const int nwaves_total = gridDim.x * SC_WAVES;
  float pm[SC_KQ], ipv[SC_KQ], lpv[SC_KQ];
#pragma unroll
  for (int q = 0; q < SC_KQ; ++q) {
    const int k = min(lane + 64 * q, K - 1);
    const float pv = a.prior_var[k];
    pm[q] = a.prior_mean[k];
    ipv[q] = 1.f / pv;
    lpv[q] = logf(pv);
  }
  for (int d = blockIdx.x * SC_WAVES + wave; d < p.n_docs; d += nwaves_total) {
    const float* mo = p.moments + (size_t)d * 2 * K;
    float mu[SC_KQ], sd[SC_KQ], kl = 0.f;
#pragma unroll
    for (int q = 0; q < SC_KQ; ++q) {
      const int k = min(lane + 64 * q, K - 1);
      mu[q] = mo[k];
      const float ls = mo[K + k];
      sd[q] = __expf(0.5f * ls);
      const float diff = pm[q] - mu[q];
      // 0.5 (sum var / pv + sum diff^2 / pv - K + sum log pv - sum log var), per topic
      const float t = (expf(ls) + diff * diff) * ipv[q] - 1.f + lpv[q] - ls;
      kl += lane + 64 * q < K ? t : 0.f;
    }
    kl = wave_sum(kl);
    if (lane == 0) p.out[2 * (size_t)d] = 0.5f * kl;

    float* trow = p.theta + (size_t)d * R * K;
    auto emit = [&](const float* z, int s) {       // softmax over the wave's K topics
      float mx = -INFINITY;
#pragma unroll
      for (int q = 0; q < SC_KQ; ++q) mx = fmaxf(mx, z[q]);
      mx = wave_max(mx);
      float e[SC_KQ], sum = 0.f;
#pragma unroll
      for (int q = 0; q < SC_KQ; ++q) {
        e[q] = lane + 64 * q < K ? __expf(z[q] - mx) : 0.f;
        sum += e[q];
      }
      const float inv = 1.f / wave_sum(sum);
#pragma unroll
      for (int q = 0; q < SC_KQ; ++q) {
        const int k = lane + 64 * q;
        if (k < K) trow[(size_t)s * K + k] = e[q] * inv;
      }
    };
    if (S <= 0) {
      float z[SC_KQ];
#pragma unroll
      for (int q = 0; q < SC_KQ; ++q) z[q] = lane + 64 * q < K ? mu[q] : -INFINITY;
      emit(z, 0);
      continue;
    }
    const uint32_t key0 = (uint32_t)((size_t)(p.doc0 + d) * K);
    for (int s0 = 0; s0 < S; s0 += 4) {
      float nz[SC_KQ][4];
#pragma unroll
      for (int q = 0; q < SC_KQ; ++q) {
        if (64 * q < K) {
          randn4(p.seed, (uint32_t)(s0 >> 2), key0 + lane + 64 * q, nz[q]);
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r) nz[q][r] = 0.f;
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (s0 + r >= S) break;
        float z[SC_KQ];
#pragma unroll
        for (int q = 0; q < SC_KQ; ++q) z[q] = lane + 64 * q < K ? mu[q] + nz[q][r] * sd[q] : -INFINITY;
        emit(z, s0 + r);
      }
    }
  }
}

// RT: row tiles of 16 per block.  dynamic LDS: th[BR][KTS] + bt[SC_KC][SC_LDB] +
// part[SC_WAVES][BR][2]
template <int RT>
__global__ void __launch_bounds__(SC_THREADS) gfk_doc_score_k(ScoreArgs a, GfkScore p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int BR = 16 * RT;                 // rows per block
  const int tid = threadIdx.x, lane = tid & 63, wave = uniform(tid >> 6);
  const int K = a.K, V = a.V, ldb = a.ldb;
  const int KP = sc_kp(K), KTS = sc_kts(K);
  const int NCH = (KP + SC_KC - 1) / SC_KC;
  const int n_tiles = (V + SC_VB - 1) / SC_VB;
  const int NV = sc_vranges(V), tiles_per_range = (n_tiles + NV - 1) / NV;
  const int R = p.n_samples > 0 ? p.n_samples : 1;
  const int n_rows = p.n_docs * R;
  const int n_blocks = (n_rows + BR - 1) / BR;
  float* th = smem;
  float* bt = th + BR * KTS;
  float* part = bt + SC_KC * SC_LDB;
  const int col = 16 * wave + (lane & 15);    // this lane's column within a tile (MFMA roles)
  const int kq = lane >> 4;
  const int sc = tid & (SC_VB - 1), sr = tid / SC_VB;   // staging: column, first chunk row
  const float bn_eps = a.bn_eps;

  // work item = (row block, vocabulary range): ranges vary fastest, so the workgroups of
  // one dispatch wave stream different parts of beta
  for (int item = blockIdx.x; item < n_blocks * NV; item += gridDim.x) {
    const int blk = item / NV, vr = item - blk * NV;
    const int row0 = blk * BR;
    const int tile_lo = vr * tiles_per_range;
    const int n_it = max(min(n_tiles, tile_lo + tiles_per_range) - tile_lo, 0) * NCH;
    // ---- the block's theta rows (zero rows past the end, zero padding columns) ----
    for (int t = tid; t < BR * KTS; t += SC_THREADS) {
      const int r = t / KTS, k = t - r * KTS;
      const float v = p.theta[(size_t)min(row0 + r, n_rows - 1) * K + min(k, K - 1)];
      th[t] = (row0 + r < n_rows && k < K) ? v : 0.f;
    }
    float lm[RT][4], lsum[RT][4];            // online (max, sum exp) over this lane's columns
#pragma unroll
    for (int i = 0; i < RT; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) { lm[i][e] = -INFINITY; lsum[i][e] = 0.f; }

    // a chunk of beta (SC_KC topics x 64 columns) and, with a tile's first chunk, the tile's
    // running statistics: into registers one chunk ahead, so they land under the MFMAs
    float br[SC_BU], rm_n = 0.f, rv_n = 1.f;
    auto issue = [&](int tile, int ch) {
      const int c = min(tile * SC_VB + sc, V - 1);
#pragma unroll
      for (int u = 0; u < SC_BU; ++u) {
        const int k = min(ch * SC_KC + sr + SC_WAVES * u, K - 1);
        br[u] = a.beta[(size_t)k * ldb + c];
      }
      if (ch == 0) {
        const int v = min(tile * SC_VB + col, V - 1);
        rm_n = a.beta_rm[v];
        rv_n = a.beta_rv[v];
      }
    };
    if (n_it > 0) issue(tile_lo, 0);
    float rm = 0.f, rs = 0.f;
    f32x4 acc[RT];
    int tile = tile_lo, ch = 0;
#pragma unroll 1
    for (int it = 0; it < n_it; ++it) {
      const int c0 = tile * SC_VB;
      lds_barrier();                         // the previous chunk's reads of bt are done
#pragma unroll
      for (int u = 0; u < SC_BU; ++u) {
        const int kk = sr + SC_WAVES * u;
        bt[kk * SC_LDB + sc] = (ch * SC_KC + kk < K && c0 + sc < V) ? br[u] : 0.f;
      }
      if (ch == 0) {
        rm = rm_n;
        rs = rsqrtf(rv_n + bn_eps);
#pragma unroll
        for (int i = 0; i < RT; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
      lds_barrier();
      const bool last = ch == NCH - 1;
      if (it + 1 < n_it) issue(last ? tile + 1 : tile, last ? 0 : ch + 1);
      // ---- logits: every row tile x this wave's 16 columns, over the chunk's topics ----
      {
        const int kend = min(SC_KC, KP - ch * SC_KC);
        const float* bp = bt + kq * SC_LDB + col;
        const float* ap = th + (lane & 15) * KTS + ch * SC_KC + kq;
        for (int k0 = 0; k0 < kend; k0 += 4) {
          const float b = bp[k0 * SC_LDB];
#pragma unroll
          for (int i = 0; i < RT; ++i) acc[i] = mfma16x16x4(ap[i * 16 * KTS + k0], b, acc[i]);
        }
      }
      if (last) {
        // ---- batch-norm with running statistics, online sum-exp ----
        if (c0 + col < V) {                  // columns >= V of the last tile contribute nothing
#pragma unroll
          for (int i = 0; i < RT; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const float zn = (acc[i][e] - rm) * rs;
              const float d = zn - lm[i][e];
              const float ex = __expf(-fabsf(d));
              lsum[i][e] = d > 0.f ? lsum[i][e] * ex + 1.f : lsum[i][e] + ex;
              lm[i][e] = fmaxf(lm[i][e], zn);
            }
        }
        ch = 0;
        ++tile;
      } else {
        ++ch;
      }
    }

    // ---- the range's (max, sum) of every row: the 16 column lanes (shuffles), then the 4
    // waves (LDS), fixed order ----
#pragma unroll
    for (int i = 0; i < RT; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float mx = lm[i][e], sm = lsum[i][e];
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {
          const float m2 = __shfl_xor(mx, o, 64), s2 = __shfl_xor(sm, o, 64);
          lse_merge(mx, sm, m2, s2);
        }
        if ((lane & 15) == 0) {
          const int row = i * 16 + kq * 4 + e;
          part[(wave * BR + row) * 2] = mx;
          part[(wave * BR + row) * 2 + 1] = sm;
        }
      }
    lds_barrier();
    if (tid < BR) {
      float mx = part[tid * 2], sm = part[tid * 2 + 1];
#pragma unroll
      for (int w = 1; w < SC_WAVES; ++w) lse_merge(mx, sm, part[(w * BR + tid) * 2], part[(w * BR + tid) * 2 + 1]);
      if (row0 + tid < n_rows) {
        float* o = p.lse_part + ((size_t)vr * n_rows + row0 + tid) * 2;
        o[0] = mx;
        o[1] = sm;
      }
    }
    lds_barrier();                           // th / part are rewritten by the next item
  }
}

// The sparse term: one wave per row.  lse[row] = the vocabulary ranges' (max, sum) pairs
// merged in range order; each lane takes non-zeros e0 + lane, + 64, ... of the row's
// document and recomputes their BN'ed logits from the theta row (LDS) and beta's column (K
// independent scattered loads each); the lanes' sums are reduced with fixed-order shuffles.
__global__ void __launch_bounds__(SC_THREADS) gfk_score_sparse_k(ScoreArgs a, GfkScore p) {
  __shared__ float ts[SC_WAVES][64 * SC_KQ];
  const int lane = threadIdx.x & 63, wave = uniform(threadIdx.x >> 6);
  const int K = a.K, ldb = a.ldb, NV = sc_vranges(a.V);
  const int R = p.n_samples > 0 ? p.n_samples : 1;
  const int n_rows = p.n_docs * R;
  const float bn_eps = a.bn_eps;
  float* trow = ts[wave];
  for (int row = blockIdx.x * SC_WAVES + wave; row < n_rows; row += gridDim.x * SC_WAVES) {
    for (int k = lane; k < K; k += 64) trow[k] = p.theta[(size_t)row * K + k];
    float mx = -INFINITY, sm = 0.f;
    for (int vr = 0; vr < NV; ++vr) {
      const float* o = p.lse_part + ((size_t)vr * n_rows + row) * 2;
      lse_merge(mx, sm, o[0], o[1]);
    }
    const float l = mx + __logf(sm);
    const int d = row / R;
    const int e0 = p.indptr[d], e1 = p.indptr[d + 1];
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     // the wave's theta row is in LDS
    __builtin_amdgcn_wave_barrier();
    float t = 0.f;
    for (int e = e0 + lane; e < e1; e += 64) {
      const int v = p.indices[e];
      const float x = p.values[e];
      const float* bc = a.beta + v;
      float z0 = 0.f, z1 = 0.f;
      int k = 0;
#pragma unroll 4
      for (; k + 2 <= K; k += 2) {
        z0 += trow[k] * bc[(size_t)k * ldb];
        z1 += trow[k + 1] * bc[(size_t)(k + 1) * ldb];
      }
      if (k < K) z0 += trow[k] * bc[(size_t)k * ldb];
      const float zn = (z0 + z1 - a.beta_rm[v]) * rsqrtf(a.beta_rv[v] + bn_eps);
      t += x * __logf(__expf(zn - l) + 1e-10f);
    }
    t = wave_sum(t);
    if (lane == 0) p.rl_rows[row] = -t;
    __builtin_amdgcn_wave_barrier();         // (trow is rewritten for the next row)
  }
}

__global__ void __launch_bounds__(SC_THREADS) gfk_score_mean_k(GfkScore p) {
  const int d = blockIdx.x * SC_THREADS + threadIdx.x;
  if (d >= p.n_docs) return;
  const int R = p.n_samples > 0 ? p.n_samples : 1;
  float t = 0.f;
  for (int s = 0; s < R; ++s) t += p.rl_rows[(size_t)d * R + s];
  p.out[2 * (size_t)d + 1] = t / (float)R;
}

template <int RT>
int launch_score(const ScoreArgs& a, const GfkScore* p, unsigned grid, size_t smem, hipStream_t s) {
  hipError_t e = hipFuncSetAttribute((const void*)gfk_doc_score_k<RT>,
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(gfk_doc_score_k<RT>, dim3(grid), dim3(SC_THREADS), smem, s, a, *p);
  return (int)hipGetLastError();
}

}  // namespace

extern "C" size_t gfk_score_struct_size() { return sizeof(GfkScore); }

// vocabulary ranges per row block (sizes GfkScore.lse_part and the decoder's grid)
extern "C" int gfk_score_vranges(const GfkModel* m) { return sc_vranges(m->V); }

// LDS bytes of the decoder kernel for this model
extern "C" size_t gfk_doc_score_smem(const GfkModel* m) { return sizeof(float) * sc_smem_floats(m->K); }

// Host checks mirror the kernels' assumptions: the ProdLDA decoder, K <= 512, a CSR with
// n_docs + 1 row pointers, n_docs * max(n_samples, 1) rows in an int, grid >= 1.
extern "C" int gfk_doc_score(const GfkModel* m, const GfkScore* p, hipStream_t s) {
  if (p->n_docs <= 0) return 0;
  if (m->kind != GFK_PRODLDA) return -2;
  if (m->K <= 0 || m->K > 64 * SC_KQ || m->V <= 0 || m->ldb < m->V || p->grid <= 0 || p->n_samples < 0 ||
      p->max_grid < 0)
    return -5;
  const int64_t R = p->n_samples > 0 ? p->n_samples : 1;
  if (R * p->n_docs >= ((int64_t)1 << 31)) return -6;
  if (!p->indptr || !p->indices || !p->values || !p->moments || !p->theta || !p->lse_part ||
      !p->rl_rows || !p->out)
    return -7;
  if (!m->beta || !m->beta_rm || !m->beta_rv || !m->prior_mean || !m->prior_var) return -8;
  ScoreArgs a;
  a.beta = m->beta; a.beta_rm = m->beta_rm; a.beta_rv = m->beta_rv;
  a.prior_mean = m->prior_mean; a.prior_var = m->prior_var;
  a.V = m->V; a.K = m->K; a.ldb = m->ldb; a.bn_eps = m->bn_eps;
  // max_grid caps the three strided launches (every result is independent of its grid);
  // gfk_score_mean_k is one thread per document with no loop and keeps its grid
  const int64_t cap = p->max_grid > 0 ? p->max_grid : ((int64_t)1 << 31);
  auto capped = [&](int64_t g) { return (unsigned)(g < cap ? g : cap); };
  const int tgrid = (int)((p->n_docs + SC_WAVES - 1) / SC_WAVES < 2048 ? (p->n_docs + SC_WAVES - 1) / SC_WAVES
                                                                       : 2048);
  hipLaunchKernelGGL(gfk_score_theta_k, dim3(capped(tgrid)), dim3(SC_THREADS), 0, s, a, *p);
  int rc = (int)hipGetLastError();
  if (rc) return rc;
  const size_t smem = gfk_doc_score_smem(m);
  const unsigned dgrid = capped(p->grid);
  rc = sc_row_tiles(m->K) == 4 ? launch_score<4>(a, p, dgrid, smem, s) : launch_score<2>(a, p, dgrid, smem, s);
  if (rc) return rc;
  const int64_t wrows = (R * p->n_docs + SC_WAVES - 1) / SC_WAVES;
  hipLaunchKernelGGL(gfk_score_sparse_k, dim3(capped(wrows < 8192 ? wrows : 8192)), dim3(SC_THREADS), 0,
                     s, a, *p);
  rc = (int)hipGetLastError();
  if (rc) return rc;
  hipLaunchKernelGGL(gfk_score_mean_k, dim3((p->n_docs + SC_THREADS - 1) / SC_THREADS), dim3(SC_THREADS), 0,
                     s, *p);
  return (int)hipGetLastError();
}
