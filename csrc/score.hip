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
//
// The NeuralLDA decoder and the label head (gfk_score_ext, second half of this file) reuse
// gfk_score_theta_k -- the same theta workspace and draw keys -- and add:
//
//   gfk_lda_topic_lse_k      L[k] = log sum_v exp(zn[k, v]), zn = (beta - rm) rsqrt(rv + eps):
//                            once per score call; (topic, vocabulary range) work items,
//                            lanes on consecutive columns (16 B per lane where the rows
//                            are 16-byte aligned), a per-lane online (max, sum) pair merged
//                            lanes -> waves -> (gfk_lda_topic_lse_fin_k) ranges in range
//                            order.  LDS: 32 B.
//   gfk_lda_sparse_k<G>      one wave per document: p[r, v] = sum_k theta[r, k]
//                            exp(zn[k, v] - L[k]) at the document's non-zeros alone, one exp
//                            per (non-zero, k) shared by a group of G draws (G = 1 for
//                            n_samples <= 1, else 4).  LDS per workgroup of 4 waves:
//                            theta [4][256 G] + L [4][256] floats = 8 KiB (G = 1) /
//                            20 KiB (G = 4).  K <= 256.
//   gfk_label_ce_k           one wave per row: logits = theta w_cls^T + b_cls, CE = lse -
//                            logit[argmax(labels)] (lowest index of the maximum).  LDS 4 KiB.
//                            K <= 256, L <= 256.
//   gfk_score_finish_k       out[d] = (KL, RL[, CE]): the draws' means in draw order.
//
// No normalised [K, V] matrix and no [rows, V] array exist.
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

// ---------------------------------------------------------------------------------------
// NeuralLDA decoder (reference decoder_network.py:121-127 in eval mode) and the label head
// (inference_network.py label_classification; avitm.py / ctm.py add its cross-entropy).
//
//   zn[k, v] = (beta[k, v] - rm[v]) rsqrt(rv[v] + bn_eps)
//   L[k]     = log sum_{v < V} exp(zn[k, v])               max-shifted: zn is unbounded
//   p[r, v]  = sum_k theta[r, k] exp(zn[k, v] - L[k])      every factor <= 1
//   RL[r]    = - sum_{v in nz(d)} x_v log(p[r, v] + 1e-10)
//   CE[r]    = lse(theta[r] w_cls^T + b_cls) - logit[argmax labels[d]]
extern "C" {
typedef struct GfkScoreX {
  GfkScore s;              // as for gfk_doc_score, but s.out is a WORKSPACE [n_docs, 2]: the
                           // theta kernel's KL and the ProdLDA decoder's RL land there
                           // (NeuralLDA does not read s.lse_part)
  const float* labels;     // [n_docs, L] the chunk's label rows; null: no CE column
  const float* topic_lse;  // [K] gfk_lda_topic_lse's L (NeuralLDA)
  float* ce_rows;          // workspace [n_docs * R] (label head)
  float* out;              // [n_docs, ncol] = (KL, RL[, CE])
  int32_t ncol, reserved;  // 2, or 3 with labels
} GfkScoreX;
}

namespace {

constexpr int LS_KMAX = 256;                 // topics of the NeuralLDA / label kernels
constexpr int TL_VEC = 4;                    // columns per lane and pass of the topic lse
constexpr int TL_STEP = SC_THREADS * TL_VEC;

struct TopicLseArgs {
  const float *beta, *rm, *rv;
  float *part, *lse;       // [NV, K, 2] (max, sum exp) partials; [K]
  int V, K, ldb, vec;      // vec: rows and statistics 16-byte aligned
  float bn_eps;
};

// Work item = (topic, vocabulary range), ranges fastest.  Thread t owns columns
// c_lo + 4 t .. + 3, + 1024, ...: the ownership -- and so every bit of the result -- is
// the same whether the four columns arrive as one 16-byte load or as four.
__global__ void __launch_bounds__(SC_THREADS) gfk_lda_topic_lse_k(TopicLseArgs a) {
  __shared__ float pm[SC_WAVES], ps[SC_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = uniform(tid >> 6);
  const int V = a.V, K = a.K;
  const int n_tiles = (V + SC_VB - 1) / SC_VB;
  const int NV = sc_vranges(V), tiles_per_range = (n_tiles + NV - 1) / NV;
  const float bn_eps = a.bn_eps;
  for (int item = blockIdx.x; item < K * NV; item += gridDim.x) {
    const int k = item / NV, vr = item - k * NV;
    const int c_lo = min(vr * tiles_per_range * SC_VB, V);
    const int c_hi = min(c_lo + tiles_per_range * SC_VB, V);
    const float* brow = a.beta + (size_t)k * a.ldb;
    float m = -INFINITY, s = 0.f;
    for (int c = c_lo + TL_VEC * tid; c < c_hi; c += TL_STEP) {
      float b[TL_VEC], rm[TL_VEC], rv[TL_VEC];
      if (a.vec && c + TL_VEC <= c_hi) {
        const float4 b4 = *reinterpret_cast<const float4*>(brow + c);
        const float4 m4 = *reinterpret_cast<const float4*>(a.rm + c);
        const float4 v4 = *reinterpret_cast<const float4*>(a.rv + c);
        b[0] = b4.x; b[1] = b4.y; b[2] = b4.z; b[3] = b4.w;
        rm[0] = m4.x; rm[1] = m4.y; rm[2] = m4.z; rm[3] = m4.w;
        rv[0] = v4.x; rv[1] = v4.y; rv[2] = v4.z; rv[3] = v4.w;
      } else {
#pragma unroll
        for (int i = 0; i < TL_VEC; ++i) {
          const int ci = min(c + i, c_hi - 1);
          b[i] = brow[ci];
          rm[i] = a.rm[ci];
          rv[i] = a.rv[ci];
        }
      }
#pragma unroll
      for (int i = 0; i < TL_VEC; ++i) {
        if (c + i < c_hi) {
          const float zn = (b[i] - rm[i]) * rsqrtf(rv[i] + bn_eps);
          const float d = zn - m;
          const float ex = __expf(-fabsf(d));
          s = d > 0.f ? s * ex + 1.f : s + ex;
          m = fmaxf(m, zn);
        }
      }
    }
    wave_lse(m, s);
    if (lane == 0) { pm[wave] = m; ps[wave] = s; }
    lds_barrier();
    if (tid == 0) {
#pragma unroll
      for (int w = 1; w < SC_WAVES; ++w) lse_merge(m, s, pm[w], ps[w]);
      float* o = a.part + ((size_t)vr * K + k) * 2;
      o[0] = m;
      o[1] = s;
    }
    lds_barrier();                           // pm / ps are rewritten by the next item
  }
}

__global__ void __launch_bounds__(SC_THREADS) gfk_lda_topic_lse_fin_k(TopicLseArgs a) {
  const int k = blockIdx.x * SC_THREADS + threadIdx.x;
  if (k >= a.K) return;
  const int NV = sc_vranges(a.V);
  float m = -INFINITY, s = 0.f;
  for (int vr = 0; vr < NV; ++vr) {
    const float* o = a.part + ((size_t)vr * a.K + k) * 2;
    lse_merge(m, s, o[0], o[1]);
  }
  a.lse[k] = m + __logf(s);
}

// One wave per document; the draws in groups of G.  th[k][g]: the group's theta (zero rows
// past the last draw), so one topic's G factors are one LDS read; lw[k] = L[k].  Each lane
// takes non-zeros e0 + lane, + 64, ...: K scattered loads of beta's column (stride ldb), one
// exp each, G multiply-adds.  (zn is the expression of gfk_lda_topic_lse_k, bit for bit.)
template <int G>
__global__ void __launch_bounds__(SC_THREADS) gfk_lda_sparse_k(ScoreArgs a, GfkScore p,
                                                               const float* __restrict__ topic_lse) {
  __shared__ __attribute__((aligned(16))) float ths[SC_WAVES][LS_KMAX * G];
  __shared__ float lws[SC_WAVES][LS_KMAX];
  const int lane = threadIdx.x & 63, wave = uniform(threadIdx.x >> 6);
  const int K = a.K, ldb = a.ldb;
  const int R = p.n_samples > 0 ? p.n_samples : 1;
  const float bn_eps = a.bn_eps;
  float* th = ths[wave];
  float* lw = lws[wave];
  for (int k = lane; k < K; k += 64) lw[k] = topic_lse[k];
  for (int d = blockIdx.x * SC_WAVES + wave; d < p.n_docs; d += gridDim.x * SC_WAVES) {
    const int e0 = p.indptr[d], e1 = p.indptr[d + 1];
    for (int s0 = 0; s0 < R; s0 += G) {
      __builtin_amdgcn_wave_barrier();       // (the previous group's reads of th are done)
      for (int k = lane; k < K; k += 64) {
#pragma unroll
        for (int g = 0; g < G; ++g) {
          const int s = min(s0 + g, R - 1);
          const float v = p.theta[((size_t)d * R + s) * K + k];
          th[k * G + g] = s0 + g < R ? v : 0.f;
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the wave's theta group is in LDS
      __builtin_amdgcn_wave_barrier();
      float t[G];
#pragma unroll
      for (int g = 0; g < G; ++g) t[g] = 0.f;
      for (int e = e0 + lane; e < e1; e += 64) {
        const int v = p.indices[e];
        const float x = p.values[e];
        const float rm = a.beta_rm[v], rs = rsqrtf(a.beta_rv[v] + bn_eps);
        const float* bc = a.beta + v;
        float pr[G];
#pragma unroll
        for (int g = 0; g < G; ++g) pr[g] = 0.f;
#pragma unroll 4
        for (int k = 0; k < K; ++k) {
          const float zn = (bc[(size_t)k * ldb] - rm) * rs;
          const float ex = __expf(zn - lw[k]);
#pragma unroll
          for (int g = 0; g < G; ++g) pr[g] += th[k * G + g] * ex;
        }
#pragma unroll
        for (int g = 0; g < G; ++g) t[g] += x * __logf(pr[g] + 1e-10f);
      }
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const float tg = wave_sum(t[g]);
        if (lane == 0 && s0 + g < R) p.rl_rows[(size_t)d * R + s0 + g] = -tg;
      }
    }
  }
}

// One wave per row; lane l owns labels l, l + 64, l + 128, l + 192.
__global__ void __launch_bounds__(SC_THREADS) gfk_label_ce_k(ScoreArgs a, GfkScore p,
                                                             const float* __restrict__ labels,
                                                             const float* __restrict__ w_cls,
                                                             const float* __restrict__ b_cls,
                                                             float* __restrict__ ce_rows, int L) {
  __shared__ float ts[SC_WAVES][LS_KMAX];
  constexpr int LQ = 4;
  const int lane = threadIdx.x & 63, wave = uniform(threadIdx.x >> 6);
  const int K = a.K;
  const int R = p.n_samples > 0 ? p.n_samples : 1;
  const int n_rows = p.n_docs * R;
  float* trow = ts[wave];
  float bias[LQ];
#pragma unroll
  for (int q = 0; q < LQ; ++q) bias[q] = b_cls[min(lane + 64 * q, L - 1)];
  for (int row = blockIdx.x * SC_WAVES + wave; row < n_rows; row += gridDim.x * SC_WAVES) {
    __builtin_amdgcn_wave_barrier();         // (the previous row's reads of trow are done)
    for (int k = lane; k < K; k += 64) trow[k] = p.theta[(size_t)row * K + k];
    // the target: the lowest index of the label row's maximum
    const float* lab = labels + (size_t)(row / R) * L;
    float bv = -INFINITY;
    int bi = 0x7fffffff;
#pragma unroll
    for (int q = 0; q < LQ; ++q) {
      const int l = lane + 64 * q;
      const float v = lab[min(l, L - 1)];
      if (l < L && v > bv) { bv = v; bi = l; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     // the wave's theta row is in LDS
    __builtin_amdgcn_wave_barrier();
    float z[LQ], mx = -INFINITY, zt = 0.f;
#pragma unroll
    for (int q = 0; q < LQ; ++q) {
      const int l = lane + 64 * q;
      const float* wr = w_cls + (size_t)min(l, L - 1) * K;
      float acc = bias[q];
      for (int k = 0; k < K; ++k) acc += trow[k] * wr[k];
      z[q] = l < L ? acc : -INFINITY;
      mx = fmaxf(mx, z[q]);
      zt += l == bi ? acc : 0.f;
    }
    mx = wave_max(mx);
    float sum = 0.f;
#pragma unroll
    for (int q = 0; q < LQ; ++q) sum += lane + 64 * q < L ? __expf(z[q] - mx) : 0.f;
    sum = wave_sum(sum);
    zt = wave_sum(zt);
    if (lane == 0) ce_rows[row] = mx + __logf(sum) - zt;
  }
}

// out[d] = (KL, RL[, CE]).  lda: RL is the mean of rl_rows in draw order (as
// gfk_score_mean_k takes it), else the ProdLDA launch's own, from the workspace.
__global__ void __launch_bounds__(SC_THREADS) gfk_score_finish_k(GfkScoreX x, int lda) {
  const int d = blockIdx.x * SC_THREADS + threadIdx.x;
  if (d >= x.s.n_docs) return;
  const int R = x.s.n_samples > 0 ? x.s.n_samples : 1;
  float* o = x.out + (size_t)d * x.ncol;
  o[0] = x.s.out[2 * (size_t)d];
  if (lda) {
    float t = 0.f;
    for (int s = 0; s < R; ++s) t += x.s.rl_rows[(size_t)d * R + s];
    o[1] = t / (float)R;
  } else {
    o[1] = x.s.out[2 * (size_t)d + 1];
  }
  if (x.ncol == 3) {
    float t = 0.f;
    for (int s = 0; s < R; ++s) t += x.ce_rows[(size_t)d * R + s];
    o[2] = t / (float)R;
  }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" size_t gfk_scorex_struct_size() { return sizeof(GfkScoreX); }

// L[k] of the eval-mode NeuralLDA decoder into lse [K]; part: workspace
// [gfk_score_vranges(V), K, 2].  Depends on the model alone: once per score call.
extern "C" int gfk_lda_topic_lse(const GfkModel* m, float* part, float* lse, int max_grid, hipStream_t s) {
  if (m->K <= 0 || m->K > LS_KMAX || m->V <= 0 || m->ldb < m->V || max_grid < 0) return -5;
  if (!part || !lse) return -7;
  if (!m->beta || !m->beta_rm || !m->beta_rv) return -8;
  TopicLseArgs a;
  a.beta = m->beta; a.rm = m->beta_rm; a.rv = m->beta_rv;
  a.part = part; a.lse = lse;
  a.V = m->V; a.K = m->K; a.ldb = m->ldb; a.bn_eps = m->bn_eps;
  a.vec = (m->ldb % TL_VEC == 0) && aligned16(m->beta) && aligned16(m->beta_rm) && aligned16(m->beta_rv);
  int grid = m->K * sc_vranges(m->V);
  if (max_grid > 0 && grid > max_grid) grid = max_grid;
  hipLaunchKernelGGL(gfk_lda_topic_lse_k, dim3(grid), dim3(SC_THREADS), 0, s, a);
  int rc = (int)hipGetLastError();
  if (rc) return rc;
  hipLaunchKernelGGL(gfk_lda_topic_lse_fin_k, dim3((m->K + SC_THREADS - 1) / SC_THREADS), dim3(SC_THREADS),
                     0, s, a);
  return (int)hipGetLastError();
}

// (KL, RL[, CE]) of a chunk on either decoder.  ProdLDA: gfk_doc_score into the workspace
// x->s.out, then the label head (plain ProdLDA has gfk_doc_score itself).  NeuralLDA: the
// theta kernel, then the sparse term against x->topic_lse.  Host checks as gfk_doc_score's.
extern "C" int gfk_score_ext(const GfkModel* m, const GfkScoreX* x, hipStream_t s) {
  const GfkScore* p = &x->s;
  if (p->n_docs <= 0) return 0;
  const bool lda = m->kind != GFK_PRODLDA;
  const bool ce = x->labels != nullptr;
  if (m->K <= 0 || m->K > LS_KMAX || m->V <= 0 || m->ldb < m->V || p->grid <= 0 || p->n_samples < 0 ||
      p->max_grid < 0 || x->ncol != (ce ? 3 : 2) || (ce && (m->L <= 0 || m->L > 256)))
    return -5;
  if (!lda && !ce) return -2;                // plain ProdLDA: gfk_doc_score
  const int64_t R = p->n_samples > 0 ? p->n_samples : 1;
  if (R * p->n_docs >= ((int64_t)1 << 31)) return -6;
  if (!p->indptr || !p->indices || !p->values || !p->moments || !p->theta || !p->rl_rows || !p->out ||
      !x->out || (lda && !x->topic_lse) || (!lda && !p->lse_part) || (ce && !x->ce_rows))
    return -7;
  if (!m->beta || !m->beta_rm || !m->beta_rv || !m->prior_mean || !m->prior_var ||
      (ce && (!m->w_cls || !m->b_cls)))
    return -8;
  ScoreArgs a;
  a.beta = m->beta; a.beta_rm = m->beta_rm; a.beta_rv = m->beta_rv;
  a.prior_mean = m->prior_mean; a.prior_var = m->prior_var;
  a.V = m->V; a.K = m->K; a.ldb = m->ldb; a.bn_eps = m->bn_eps;
  const int64_t cap = p->max_grid > 0 ? p->max_grid : ((int64_t)1 << 31);
  auto capped = [&](int64_t g) { return (unsigned)(g < cap ? g : cap); };
  const int64_t wdocs = (p->n_docs + SC_WAVES - 1) / SC_WAVES;
  const int64_t wrows = (R * p->n_docs + SC_WAVES - 1) / SC_WAVES;
  int rc;
  if (lda) {
    hipLaunchKernelGGL(gfk_score_theta_k, dim3(capped(wdocs < 2048 ? wdocs : 2048)), dim3(SC_THREADS), 0, s,
                       a, *p);
    rc = (int)hipGetLastError();
    if (rc) return rc;
    const dim3 g(capped(wdocs < 8192 ? wdocs : 8192));
    if (R == 1) hipLaunchKernelGGL(gfk_lda_sparse_k<1>, g, dim3(SC_THREADS), 0, s, a, *p, x->topic_lse);
    else hipLaunchKernelGGL(gfk_lda_sparse_k<4>, g, dim3(SC_THREADS), 0, s, a, *p, x->topic_lse);
    rc = (int)hipGetLastError();
  } else {
    rc = gfk_doc_score(m, p, s);
  }
  if (rc) return rc;
  if (ce) {
    hipLaunchKernelGGL(gfk_label_ce_k, dim3(capped(wrows < 8192 ? wrows : 8192)), dim3(SC_THREADS), 0, s, a,
                       *p, x->labels, (const float*)m->w_cls, (const float*)m->b_cls, x->ce_rows, (int)m->L);
    rc = (int)hipGetLastError();
    if (rc) return rc;
  }
  hipLaunchKernelGGL(gfk_score_finish_k, dim3((p->n_docs + SC_THREADS - 1) / SC_THREADS), dim3(SC_THREADS), 0,
                     s, *x, lda ? 1 : 0);
  return (int)hipGetLastError();
}
