// The optimizer step of every encoder tensor, each fused with the kernel that
// completes its gradient, plus the next-batch prep.  Workgroup roles:
//   [0, n_tiles)         W_in tiles (below)
//   [n_tiles, +n_w)      small weight tiles: G[j][i] = sum_b dz[b][j] a[b][i] for a
//                        64 x 64 output tile of W_h[l] / W_mu / W_s (MFMA, fused Adam)
//   [.., +n_v)           bias / prior vectors: column sums over the batch (16 lanes
//                        per column, DPP reduction) or the prior gradient, fused Adam
//   last                 prepare_next_batch
// (beta is updated in prodlda_bwd's epilogue.)
//
// dW_in^T[v, :] = sum_b x[b, v] dz0[b, :]  (reference: autograd of
// inference_network.py:76 input_layer).  W_in is stored transposed ([V, H0]), so
// a vocabulary tile of 64 words is a contiguous [64, H0] block.  Instead of
// scattering B * nnz rows with float atomics (order-dependent, and each wave
// serialises on its outstanding-atomic budget), every workgroup owns one tile:
//   * builds the dense x^T tile [64, B] in LDS from the per-row tile start table
//     (ws_tstart, written by enc_in) -- the CSR non-zeros of the tile;
//   * multiplies it with dz0 [B, H0] on the fp32 matrix cores (16 waves, one
//     16x16 output tile each at H0 <= 64);
//   * applies Adam (and the FedAvg pre-scale) to its W_in block in the epilogue,
//     with p / m / v prefetched before the MFMA (fused mode), or stores the
//     gradient (gradient mode).
// Deterministic, no atomics, W_in's gradient is never materialised in fused mode.
// One extra workgroup prepares the next minibatch (gfk_common.h).
#define GFK_BATCHED_COPY 1   // batched kernels copy their descriptor (gfk_common.h gfk_model)
#include <type_traits>

#include "gfk_common.h"
#include "gfk_launch.h"

using namespace gfk;

namespace {
// Workgroup size UT: 16 waves when the grid fits the CUs (one round of workgroups: the
// most waves per tile, the shortest critical path -- the K=50 headline); 8 waves for
// large vocabularies, where the W_in tiles ([64, H0] blocks, 16 MFMA subtiles at H0 <= 64)
// outnumber the CUs several times: four workgroups share a CU and one's staging round
// overlaps another's MFMAs and stores.
__host__ __device__ inline int rup(int x, int m) { return (x + m - 1) / m * m; }
// LDS strides for ds_read_b32 MFMA operands (bank = dword % 32 per half-wave):
// A-role reads (lane & 15 -> row, lane >> 4 -> k) want stride = 2 x odd, so 16 rows x
// 2 k land on 32 distinct banks; B-role reads (lane >> 4 -> row, lane & 15 -> column)
// want stride = 16 mod 32, so a half-wave's 2 rows x 16 columns do.
__host__ __device__ inline int stride_a(int w) {
  int s = rup(w, 2);
  if ((s / 2) % 2 == 0) s += 2;
  return s;
}
__host__ __device__ inline int stride_b(int w) {   // w: multiple of 16
  return w % 32 == 16 ? w : w + 16;
}
}  // namespace

// weight jobs stage the batch in chunks of at most WJ_ROWS rows (large batches: several)
constexpr int WJ_ROWS = 128;

extern "C" size_t gfk_win_update_smem(const GfkModel* m) {
  const int B = m->bmax, H0P = rup(m->H[0], 16);
  // (the dense x^T tile path does not run at bmax > 128: the large-batch plan always takes
  // the sparse tiles)
  // (bmax > 128: the chunked dense tile, 128 rows at a time, win_tile_dense_ch)
  const int BR = B > WJ_ROWS ? WJ_ROWS : B;
  size_t a = (size_t)64 * stride_a(BR) + (size_t)BR * stride_b(H0P);
  const size_t b = 2 * (size_t)(B < WJ_ROWS ? B : WJ_ROWS) * 80;
  if (a < 64 * 64) a = 64 * 64;      // the flat epilogue's gradient tile [64, H0 <= 64]
  // the sparse tile (bit 4): dz0, the entry list, the row slots (+ the word mask and list)
  const size_t c = (size_t)B * m->H[0] + 2 * 512 + (B + 1 > 129 ? B + 1 : 129) + 128;
  if (a < c) a = c;
  // the dense contextual tile next to them (fused CombinedTM): dz0 + the A block / G tile,
  // rows at the padded stride (80 floats, win_tile_ctx)
  const size_t d = (size_t)B * 80 +
                   ((size_t)B * 80 > (size_t)64 * m->H[0] ? (size_t)B * 80 : (size_t)64 * m->H[0]);
  if (m->input == GFK_IN_COMBINED && a < d) a = d;
  return sizeof(float) * (a > b ? a : b);
}

// Small weight tile job (see GfkWJob).  LDS: dz[B][LDJ] + a[B][LDJ]
template <int UT, bool GB = false>
__device__ __forceinline__ void weight_job(const GfkModel& m, const GfkWJob& J, float* smem) {
  constexpr int UW = UT / 64;
  constexpr int LDJ = 80;            // B-role stride (16 mod 32): conflict-free operand reads
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int B = m.bmax, nb = *m.ws_nb;
  float* dzs = smem;
  float* as = smem + B * LDJ;
  const bool fused = m.update_mode == 1;
  // prefetch: the lane's 4 outputs of subtiles (jt, it) = (t >> 2, t & 3), t = wave + UW u
  constexpr int WU = 16 / UW;
  float pp[WU][4], pm[WU][4], pv[WU][4];
#pragma unroll
  for (int u = 0; u < WU; ++u) {
    const int t = wave + UW * u, jt = t >> 2, it = t & 3;
    const int i = J.i0 + it * 16 + (lane & 15);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int j = J.j0 + jt * 16 + (lane >> 4) * 4 + r;
      const float* p = J.param + (size_t)min(j, J.rows - 1) * J.cols + min(i, J.cols - 1);
      pp[u][r] = pm[u][r] = pv[u][r] = 0.f;
      if (fused) { pp[u][r] = *p; pm[u][r] = p[m.off_m]; pv[u][r] = p[m.off_v]; }
    }
  }
  // stage the two [B x 64] column slices (rows >= nb zero)
  for (int e0 = 0; e0 < B * 64; e0 += 4 * UT) {
    float vz[4], va[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int e = e0 + u * UT + tid, b = min(e >> 6, B - 1), c = e & 63;
      vz[u] = J.dz[(size_t)b * J.rows + min(J.j0 + c, J.rows - 1)];
      va[u] = J.a[(size_t)b * J.cols + min(J.i0 + c, J.cols - 1)];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int e = e0 + u * UT + tid, b = e >> 6, c = e & 63;
      if (b < B) {
        dzs[b * LDJ + c] = (b < nb && J.j0 + c < J.rows) ? vz[u] : 0.f;
        as[b * LDJ + c] = (b < nb && J.i0 + c < J.cols) ? va[u] : 0.f;
      }
    }
  }
  lds_barrier();
  const AdamCoef ac = adam_coef(m);
  const bool sh = is_shared(m, J.param);
#pragma unroll
  for (int u = 0; u < WU; ++u) {
    const int t = wave + UW * u, jt = t >> 2, it = t & 3;
    const int i = J.i0 + it * 16 + (lane & 15);
    const float* ap = dzs + (lane >> 4) * LDJ + jt * 16 + (lane & 15);
    const float* bp = as + (lane >> 4) * LDJ + it * 16 + (lane & 15);
    f32x4 c0 = {0.f, 0.f, 0.f, 0.f}, c1 = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < B; k += 8) {
      c0 = mfma16x16x4(ap[k * LDJ], bp[k * LDJ], c0);
      c1 = mfma16x16x4(ap[(k + 4) * LDJ], bp[(k + 4) * LDJ], c1);
    }
    const f32x4 g = c0 + c1;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int j = J.j0 + jt * 16 + (lane >> 4) * 4 + r;
      if (j >= J.rows || i >= J.cols) continue;
      float* p = J.param + (size_t)j * J.cols + i;
      if (!fused) {
        p[m.off_g] = g[r];
      } else {
        float mo = pm[u][r], vo = pv[u][r];
        float np = adam_update(pp[u][r], g[r], mo, vo, ac);
        if (sh && m.fed_scale_on) np *= m.fed_scale;
        p[m.off_m] = mo;
        p[m.off_v] = vo;
        p[gfk_own<GB>(m)] = np;
      }
    }
  }
}

// The large-batch plan's weight job (bmax > WJ_ROWS, gradient mode): the two [B x 64] column
// slices staged WJ_ROWS rows at a time, the MFMA accumulators carried over the chunks, the
// gradient stored.  LDS: dz[WJ_ROWS][LDJ] + a[WJ_ROWS][LDJ]
template <int UT>
__device__ __forceinline__ void weight_job_lb(const GfkModel& m, const GfkWJob& J, float* smem) {
  constexpr int UW = UT / 64, WU = 16 / UW;
  constexpr int LDJ = 80;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int B = m.bmax, nb = *m.ws_nb;
  float* dzs = smem;
  float* as = smem + WJ_ROWS * LDJ;
  f32x4 c0[WU], c1[WU];
#pragma unroll
  for (int u = 0; u < WU; ++u) c0[u] = c1[u] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int b0 = 0; b0 < B; b0 += WJ_ROWS) {
    if (b0) lds_barrier();             // the previous chunk's operand reads are done
    for (int e0 = 0; e0 < WJ_ROWS * 64; e0 += 4 * UT) {
      float vz[4], va[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int e = e0 + u * UT + tid, b = b0 + (e >> 6), c = e & 63;
        vz[u] = J.dz[(size_t)b * J.rows + min(J.j0 + c, J.rows - 1)];
        va[u] = J.a[(size_t)b * J.cols + min(J.i0 + c, J.cols - 1)];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int e = e0 + u * UT + tid, bl = e >> 6, b = b0 + bl, c = e & 63;
        dzs[bl * LDJ + c] = (b < nb && J.j0 + c < J.rows) ? vz[u] : 0.f;
        as[bl * LDJ + c] = (b < nb && J.i0 + c < J.cols) ? va[u] : 0.f;
      }
    }
    lds_barrier();
#pragma unroll
    for (int u = 0; u < WU; ++u) {
      const int t = wave + UW * u, jt = t >> 2, it = t & 3;
      const float* ap = dzs + (lane >> 4) * LDJ + jt * 16 + (lane & 15);
      const float* bp = as + (lane >> 4) * LDJ + it * 16 + (lane & 15);
      for (int k = 0; k < WJ_ROWS; k += 8) {
        c0[u] = mfma16x16x4(ap[k * LDJ], bp[k * LDJ], c0[u]);
        c1[u] = mfma16x16x4(ap[(k + 4) * LDJ], bp[(k + 4) * LDJ], c1[u]);
      }
    }
  }
#pragma unroll
  for (int u = 0; u < WU; ++u) {
    const int t = wave + UW * u, jt = t >> 2, it = t & 3;
    const int i = J.i0 + it * 16 + (lane & 15);
    const f32x4 g = c0[u] + c1[u];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int j = J.j0 + jt * 16 + (lane >> 4) * 4 + r;
      if (j < J.rows && i < J.cols) J.param[(size_t)j * J.cols + i + m.off_g] = g[r];
    }
  }
}

// Vector job (see GfkVJob): 16 lanes per element split the batch rows.  LB: the large-batch
// instance (rows in passes of 128)
template <int UT, bool LB = false, bool GB = false>
__device__ __forceinline__ void vector_job(const GfkModel& m, const GfkVJob& J) {
  const int tid = threadIdx.x, s = tid & 15;
  const int B = m.bmax, nb = *m.ws_nb;
  const bool fused = m.update_mode == 1;
  const AdamCoef ac = adam_coef(m);
  const bool sh = is_shared(m, J.param);
  for (int c0 = 0; c0 < J.n; c0 += UT / 16) {
    const int c = c0 + (tid >> 4), cc = min(c, J.n - 1);
    float* p = J.param + cc;
    float pp = 0.f, pm = 0.f, pv = 0.f, g = 0.f;
    if (fused) { pp = *p; pm = p[m.off_m]; pv = p[m.off_v]; }
    if (J.src) {
      constexpr int RU = 8;                  // 8 rows per lane per pass (LB: B / 128 passes)
      float v[RU];
#pragma unroll
      for (int u = 0; u < RU; ++u) v[u] = J.src[(size_t)min(s + 16 * u, B - 1) * J.n + cc];
#pragma unroll
      for (int u = 0; u < RU; ++u) g += s + 16 * u < nb ? v[u] : 0.f;
      if constexpr (LB) {
        for (int r0 = 16 * RU; r0 < B; r0 += 16 * RU) {
#pragma unroll
          for (int u = 0; u < RU; ++u) v[u] = J.src[(size_t)min(r0 + s + 16 * u, B - 1) * J.n + cc];
#pragma unroll
          for (int u = 0; u < RU; ++u) g += r0 + s + 16 * u < nb ? v[u] : 0.f;
        }
      }
      g = row16_sum(g);
    } else {
      g = p[m.off_g];
    }
    if (s != 0 || c >= J.n) continue;
    if (!fused) {
      if (J.src) p[m.off_g] = g;
    } else {
      float np = adam_update(pp, g, pm, pv, ac);
      if (sh && m.fed_scale_on) np *= m.fed_scale;
      p[m.off_m] = pm;
      p[m.off_v] = pv;
      p[gfk_own<GB>(m)] = np;
    }
  }
}

// Sparse W_in tile (stage_flags bit 4, large vocabularies: a 64-word tile holds only a
// few of the batch's non-zeros, ~7 at V = 112k).  The dense x^T tile + MFMA GEMM of the
// default path spends its staging on zero-filling and scattering a mostly empty [64, B]
// tile; here the tile's non-zeros become an entry list (rows in order, CSR order within a
// row: a scan of the rows' counts gives every row its slot range) and every thread
// accumulates its own elements of the flat [64, H0] block over the list,
//   G[v, h] = sum_{entries (b, v, x), b ascending} x dz0[b, h],
// a fixed order (deterministic, no atomics).  The W_in / m / v block moves as flat quads
// (one round, issued first); Adam (+ FedAvg pre-scale) or the gradient store follows.
// More entries than CAP are taken in passes of CAP (each thread's sums stay in registers).
constexpr int WIN_SPARSE = 16;
constexpr int WIN_BATCH8 = 512;
// VL: the second moment goes through LDS (one LDS-DMA copy of the block, issued with the
// other staging loads) instead of 2 quads of registers per thread, so the tile fits 64
// VGPRs and 4 workgroups per CU (fused mode; the launcher picks it when the block fits the
// kernel's existing LDS budget)
// RS: row slots per thread (64 rows each): 2 up to bmax = 128, GFK_BMAX_LIMIT / 64 for the
// large-batch plan
template <int UT, bool VL = false, int RS = 2, bool GB = false>
__device__ __forceinline__ void win_tile_sparse(const GfkModel& m, float* smem, int tile) {
  constexpr int CAP = 512;
  constexpr int TPR = UT / 64;                 // threads per row, 64 rows per pass
  constexpr int FQ = 64 * 64 / 4 / UT;         // quads per thread (H0 <= 64)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int B = m.bmax, H0 = m.H[0], V = m.V, c0 = tile * 64;
  const int nb = *m.ws_nb;
  float* dz = smem;                            // [B][H0]
  int* ecol = reinterpret_cast<int*>(dz + B * H0);   // [CAP] (row << 8) | local column
  float* ex = reinterpret_cast<float*>(ecol + CAP);  // [CAP]
  int* offs = reinterpret_cast<int*>(ex + CAP);      // [64 RS + 1] rows' first slots, total
  float* vb = smem + ((B * H0 + 2 * CAP + 64 * RS + 1 + 3) & ~3);  // VL: [64 * H0] second moment
  float* wblk = m.w_in + (size_t)c0 * H0;
  const int nel = (min(V, c0 + 64) - c0) * H0;
  const bool fused = m.update_mode == 1;
  const bool al4 = ((uintptr_t)wblk % 16 == 0) && m.off_m % 4 == 0 && m.off_v % 4 == 0 &&
                   m.off_g % 4 == 0;
  auto ld4 = [&](const float* q, int e) {
    if (al4 && e + 3 < nel) return *reinterpret_cast<const f32x4*>(q + e);
    f32x4 r;
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = e + i < nel ? q[e + i] : 0.f;
    return r;
  };
  // ---- one staging round.  Issue order matters (vmcnt counts in order): the rows' tile
  // extents first, so the dependent first-entry loads wait for them alone while the
  // block's p / m / v quads and dz0 stay in flight ----
  const int32_t* tst = m.ws_tstart;
  const int ntp = m.n_tiles + 1;
  const int sub = tid % TPR;
  int xe0[RS], xe1[RS], cnt[RS];
#pragma unroll
  for (int i = 0; i < RS; ++i) {             // rows tid / TPR (+ 64 i): the entry loads
    const int r = min(tid / TPR + 64 * i, B - 1);
    xe0[i] = tst[(size_t)r * ntp + tile];
    xe1[i] = tst[(size_t)r * ntp + tile + 1];
  }
#pragma unroll
  for (int i = 0; i < RS; ++i) {             // wave 0: rows lane (+ 64 i): the slot scan
    const int r = min(lane + 64 * i, B - 1);
    cnt[i] = wave == 0 ? tst[(size_t)r * ntp + tile + 1] - tst[(size_t)r * ntp + tile] : 0;
  }
  __builtin_amdgcn_sched_barrier(0);
  f32x4 pp[FQ], pm[FQ], pv[VL ? 1 : FQ];
#pragma unroll
  for (int u = 0; u < FQ; ++u) {
    const int e = 4 * (tid + UT * u);
    pp[u] = pm[u] = f32x4{0.f, 0.f, 0.f, 0.f};
    if constexpr (!VL) pv[u] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (fused && e < nel) {
      pp[u] = ld4(wblk, e);
      pm[u] = ld4(wblk + m.off_m, e);
      if constexpr (!VL) pv[u] = ld4(wblk + m.off_v, e);
    }
  }
  if constexpr (VL) {
    if (!fused) {
    } else if (al4) {
      const int n4 = nel & ~3;
      glds_copy(vb, wblk + m.off_v, n4, tid, UT);
      if (tid < nel - n4) vb[n4 + tid] = wblk[m.off_v + n4 + tid];
    } else {
      for (int e = tid; e < nel; e += UT) vb[e] = wblk[m.off_v + e];
    }
  }
  glds_copy(dz, m.ws_dz[0], B * H0, tid, UT);
  __builtin_amdgcn_sched_barrier(0);
  // each thread's first entry of each of its rows (clamped, unconditional)
  int fi[RS];
  float fv[RS];
#pragma unroll
  for (int i = 0; i < RS; ++i) {
    const int e = min(xe0[i] + sub, max(xe1[i] - 1, 0));
    fi[i] = m.indices[e];
    fv[i] = m.values[e];
  }
  if (wave == 0) {             // row counts -> slots, rows in order
    int base = 0;
#pragma unroll
    for (int i = 0; i < RS; ++i) {
      const int c = lane + 64 * i < nb ? cnt[i] : 0;
      int x = c;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const int y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
      }
      offs[lane + 64 * i] = base + x - c;
      base += __shfl(x, 63, 64);
    }
    if (lane == 0) offs[64 * RS] = base;
  }
  vm_barrier();
  const int total = offs[64 * RS];
  // this thread's quads: word (row) v0 and column h0 of the first element; a quad spans at
  // most two words (H0 >= 4): elements with h0 + i >= H0 belong to word v0 + 1
  int qv[FQ], qh[FQ];
#pragma unroll
  for (int u = 0; u < FQ; ++u) {
    const int el = 4 * (tid + UT * u);
    qv[u] = el < nel ? el / H0 : -2;
    qh[u] = el % H0;
  }
  f32x4 g[FQ];
#pragma unroll
  for (int u = 0; u < FQ; ++u) g[u] = f32x4{0.f, 0.f, 0.f, 0.f};
  // the list sums of one pass (fixed order: slots ascending)
  auto sums = [&](int n) {
    for (int j = 0; j < n; ++j) {
      const int cb = ecol[j];
      const float x = ex[j];
      const int col = cb & 255;
      const float* dr = dz + (cb >> 8) * H0;
#pragma unroll
      for (int u = 0; u < FQ; ++u) {
        const int d = col - qv[u];             // 0: this word, 1: the next one
        if (d == 0 || d == 1) {
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int h = qh[u] + i - d * H0;  // the element's column in word col
            if (h >= 0 && h < H0 && 4 * (tid + UT * u) + i < nel) g[u][i] = __builtin_fmaf(x, dr[h], g[u][i]);
          }
        }
      }
    }
  };
  // pass 0 from the staged registers (the first entries are already loaded); later passes
  // (more than CAP entries in the tile) re-read the rows' extents, so neither the extents
  // nor the first entries stay live across the sums
#pragma unroll
  for (int i = 0; i < RS; ++i) {
    const int r = tid / TPR + 64 * i;
    if (r >= nb) continue;
    const int o = offs[r] - xe0[i];
    int e = xe0[i] + sub;
    if (e < xe1[i] && o + e < CAP) {
      ecol[o + e] = (r << 8) | (fi[i] - c0);
      ex[o + e] = fv[i];
    }
    for (e += TPR; e < xe1[i] && o + e < CAP; e += TPR) {   // (rows with more than TPR entries)
      ecol[o + e] = (r << 8) | (m.indices[e] - c0);
      ex[o + e] = m.values[e];
    }
  }
  __syncthreads();
  sums(min(CAP, total));
  for (int p0 = CAP; p0 < total; p0 += CAP) {
    __syncthreads();                           // the previous pass's list reads are done
#pragma unroll
    for (int i = 0; i < RS; ++i) {
      const int r = tid / TPR + 64 * i;
      if (r >= nb) continue;
      const int a0 = tst[(size_t)r * ntp + tile], a1 = tst[(size_t)r * ntp + tile + 1];
      const int o = offs[r] - a0;
      for (int e = a0 + sub; e < a1; e += TPR) {
        const int s = o + e - p0;
        if (s >= 0 && s < CAP) {
          ecol[s] = (r << 8) | (m.indices[e] - c0);
          ex[s] = m.values[e];
        }
      }
    }
    __syncthreads();
    sums(min(CAP, total - p0));
  }
  // ---- update (fused: Adam + FedAvg pre-scale) or the gradient ----
  const AdamCoef ac = adam_coef(m);
  const bool sh = is_shared(m, m.w_in);
#pragma unroll
  for (int u = 0; u < FQ; ++u) {
    const int e = 4 * (tid + UT * u);
    if (e >= nel) break;
    f32x4 np, mo, vo;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float a = pm[u][i], b;
      if constexpr (VL) b = e + i < nel ? vb[e + i] : 0.f;
      else b = pv[u][i];
      const float x = fused ? adam_update(pp[u][i], g[u][i], a, b, ac) : g[u][i];
      np[i] = sh && m.fed_scale_on && fused ? x * m.fed_scale : x;
      mo[i] = a;
      vo[i] = b;
    }
    auto st4 = [&](float* q, const f32x4& x) {
      if (al4 && e + 3 < nel) { *reinterpret_cast<f32x4*>(q + e) = x; return; }
#pragma unroll
      for (int i = 0; i < 4; ++i) if (e + i < nel) q[e + i] = x[i];
    };
    if (!fused) {
      st4(wblk + m.off_g, np);
    } else {
      st4(wblk + m.off_m, mo);
      st4(wblk + m.off_v, vo);
      st4(wblk + gfk_own<GB>(m), np);
    }
  }
}

// CombinedTM's contextual input-layer tile next to the sparse bag-of-words tiles (one
// launch, stage_flags bit 4 with ctx_fused == 1): Wc = rows V..2V-1 of the transposed
// input layer, G[v, h] = sum_{b < nb} A[b, v] dz0[b, h] with A the tile's adapted rows
// (ctx_fwd's ws_actx slab, [B][64]).  Both operand blocks arrive by LDS-DMA in their
// global layout ([B][64] and [B][H0], contiguous) -- no transposing scatter: the MFMA's
// reduction axis is b, and both roles read 16 consecutive columns of 4 rows per wave.
// The gradient tile is parked in the A block's LDS (free after the products) in the
// W block's flat order, and the epilogue moves p / m / v as flat quads prefetched before
// the products, like the sparse tile's.  B <= 64, H0 <= 64.
constexpr int WCS = 80;
template <int UT>
__device__ __forceinline__ void win_tile_ctx(const GfkModel& m, float* smem, int tile) {
  constexpr int UW = UT / 64;
  constexpr int FQ = 64 * 64 / 4 / UT;         // quads per thread (H0 <= 64)
  const int tid = threadIdx.x, lane = tid & 63, wave = uniform(tid >> 6);
  const int B = m.bmax, H0 = m.H[0], V = m.V, c0 = tile * 64;
  const int nb = *m.ws_nb;
  // operand rows at stride WCS = 80 floats (16 mod 32): a half-wave's two rows of 16 columns
  // land on 32 distinct ds_read_b32 banks -- at the blocks' own strides (64, H0 = 50) the two
  // rows shared banks, half of the LDS cycles of the MFMA loop were conflicts (CombinedTM
  // K = 100: SQ_LDS_BANK_CONFLICT 49 % of SQ_LDS_IDX_ACTIVE, profiles/r4)
  float* dz = smem;                                       // [B][WCS]
  float* at = smem + B * WCS;                             // [B][WCS], then G [64][H0]
  float* wblk = m.w_in + (size_t)(V + c0) * H0;
  const int nel = (min(V, c0 + 64) - c0) * H0;
  const bool fused = m.update_mode == 1;
  const bool al4 = ((uintptr_t)wblk % 16 == 0) && m.off_m % 4 == 0 && m.off_v % 4 == 0 &&
                   m.off_g % 4 == 0;
  auto ld4 = [&](const float* q, int e) {
    if (al4 && e + 3 < nel) return *reinterpret_cast<const f32x4*>(q + e);
    f32x4 r;
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = e + i < nel ? q[e + i] : 0.f;
    return r;
  };
  // ---- one staging round: the operand blocks (LDS-DMA, one dword per lane: a row per
  //      wave instruction, at the padded stride), then the W block's p / m / v ----
  {
    const float* ag = m.ws_actx + (size_t)tile * B * 64;
    for (int r = wave; r < B; r += UW) {
      if (lane < H0)
        __builtin_amdgcn_global_load_lds((gbl_void_ptr)(m.ws_dz[0] + r * H0 + lane),
                                         (lds_void_ptr)(dz + r * WCS), 4, 0, 0);
      __builtin_amdgcn_global_load_lds((gbl_void_ptr)(ag + r * 64 + lane),
                                       (lds_void_ptr)(at + r * WCS), 4, 0, 0);
    }
  }
  f32x4 pp[FQ], pm[FQ], pv[FQ];
#pragma unroll
  for (int u = 0; u < FQ; ++u) {
    const int e = 4 * (tid + UT * u);
    pp[u] = pm[u] = pv[u] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (fused && e < nel) {
      pp[u] = ld4(wblk, e);
      pm[u] = ld4(wblk + m.off_m, e);
      pv[u] = ld4(wblk + m.off_v, e);
    }
  }
  vm_barrier();
  // ---- G subtiles (v tile, h tile) = t = wave + UW u: rows b >= nb masked in the A role;
  //      columns h >= H0 read the row's padding (discarded outputs) ----
  const int NT = (H0 + 15) / 16, NST = 4 * NT;
  constexpr int SU = 16 / UW;                   // subtiles per wave (H0 <= 64: <= 16 in all)
  f32x4 acc[SU];
#pragma unroll
  for (int u = 0; u < SU; ++u) {
    const int t = wave + UW * u;
    acc[u] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (t >= NST) continue;
    const int i0 = (t / NT) * 16, j0 = (t % NT) * 16;
    const float* ap = at + (lane >> 4) * WCS + i0 + (lane & 15);
    const float* bp = dz + (lane >> 4) * WCS + j0 + (lane & 15);
    for (int k = 0; k < B; k += 4) {
      const float a = k + (lane >> 4) < nb ? ap[k * WCS] : 0.f;
      acc[u] = mfma16x16x4(a, bp[k * WCS], acc[u]);
    }
  }
  lds_barrier();                                // every wave is done reading the A block
#pragma unroll
  for (int u = 0; u < SU; ++u) {
    const int t = wave + UW * u;
    if (t >= NST) continue;
    const int i0 = (t / NT) * 16, j = (t % NT) * 16 + (lane & 15);
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (j < H0) at[(i0 + (lane >> 4) * 4 + r) * H0 + j] = acc[u][r];
  }
  lds_barrier();
  // ---- update (fused: Adam + FedAvg pre-scale) or the gradient, flat quads ----
  const AdamCoef ac = adam_coef(m);
  const bool sh = is_shared(m, m.w_in);
#pragma unroll
  for (int u = 0; u < FQ; ++u) {
    const int e = 4 * (tid + UT * u);
    if (e >= nel) break;
    f32x4 g;
#pragma unroll
    for (int i = 0; i < 4; ++i) g[i] = e + i < nel ? at[e + i] : 0.f;
    f32x4 np, mo, vo;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float a = pm[u][i], b = pv[u][i];
      const float x = fused ? adam_update(pp[u][i], g[i], a, b, ac) : g[i];
      np[i] = sh && m.fed_scale_on && fused ? x * m.fed_scale : x;
      mo[i] = a;
      vo[i] = b;
    }
    auto st4 = [&](float* q, const f32x4& x) {
      if (al4 && e + 3 < nel) { *reinterpret_cast<f32x4*>(q + e) = x; return; }
#pragma unroll
      for (int i = 0; i < 4; ++i) if (e + i < nel) q[e + i] = x[i];
    };
    if (!fused) {
      st4(wblk + m.off_g, np);
    } else {
      st4(wblk + m.off_m, mo);
      st4(wblk + m.off_v, vo);
      st4(wblk, np);
    }
  }
}

// grid: n_tiles + n_w + n_v + 1 (+ n_tiles for fused CombinedTM, + ceil(C / 64) for fused
// ZeroShotTM) workgroups of 1024 threads.  The trailing tiles are the contextual input
// layer: CombinedTM's Wc = rows V..2V-1 of the transposed W_in with the dense adapted
// rows A^T (ctx_fwd's output) in place of x^T, or ZeroShotTM's whole [C, H0] layer with
// the batch's contextual rows x_ctx^T -- the same tile GEMM + Adam epilogue.
// dynamic LDS: max(W_in tile: xt[64][stride_a(B)] + dz[B][stride_b(H0P)], weight job: 2 B 80)
// (8-wave shape: at most 64 VGPRs, so the 4 workgroups its 37 KB of LDS allows per CU also
// fit the register file -- the batched instance compiled to 68 VGPRs, 7 waves per SIMD)
// WPS: the waves per SIMD it is compiled for.  The 8-wave shape at 8 spills (the job paths
// alone need ~86 VGPRs); at 6 (80 VGPRs, three workgroups per CU) it does not -- the
// batched instance of stage_flags GFK_WIN_WAVES6, for launches whose workgroups three per
// CU hold at once.  That instance has a tile body of its own (the second one below), which
// stages the tile in one global round and needs the registers: at 64 VGPRs the same body
// spilled 11 and measured slower than the first one (profiles/r13/)
template <int UT, bool GB = false, int WPS = (UT == 512 ? 8 : 1)>
__global__ void __launch_bounds__(UT, WPS) gfk_win_update_k(GfkArgT<GB> ga, GfkUArgT<GB> gua) {
  const GfkModel& m = gfk_model(ga);
  const GfkUpdate& U = gfk_upd(gua);
  constexpr int UW = UT / 64;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int nt_here = m.n_tiles;
  {
    const int r = (int)gfk_bx() - nt_here;
    // (stamps of a batched launch, tools/stamps.py --clients: the first weight job, the last
    // vector job and the next-batch workgroup, slots 656 / 658 / 660 + entry, end)
    if (r >= 0 && r < U.n_w) {
      GFK_STAMP_IF(m, m.n_batch > 1 && r == 0, 656);
      weight_job<UT, GB>(m, U.w[r], smem);
      GFK_STAMP_IF_VM(m, m.n_batch > 1 && r == 0, 657);
      return;
    }
    if (r >= U.n_w && r < U.n_w + U.n_v) {
      GFK_STAMP_IF(m, m.n_batch > 1 && r == U.n_w + U.n_v - 1, 658);
      vector_job<UT, false, GB>(m, U.v[r - U.n_w]);
      GFK_STAMP_IF_VM(m, m.n_batch > 1 && r == U.n_w + U.n_v - 1, 659);
      return;
    }
    if (r == U.n_w + U.n_v) {
      GFK_STAMP_IF(m, m.n_batch > 1, 660);
      prepare_next_batch(m, reinterpret_cast<int*>(smem));
      GFK_STAMP_IF_VM(m, m.n_batch > 1, 661);
      return;
    }
  }
  if constexpr (WPS != 6) {
  // ---- the tile body of the shapes' own instances ----
    const bool zs = m.ctx_fused == 2;            // ZeroShotTM: W_in is the dense [C, H0] layer
    if (m.input == GFK_IN_CONTEXTUAL && !zs) return;   // (host GEMMs when not fused)
    const int rr = (int)gfk_bx() - (nt_here + U.n_w + U.n_v + 1);
    const bool ctxt = rr >= 0;                   // a Wc tile (CombinedTM) / W tile (ZeroShotTM)
    if (zs && !ctxt) return;                     // ZeroShotTM has no bag-of-words half
    const int tid = threadIdx.x, lane = tid & 63, wave = uniform(tid >> 6);
    int B = m.bmax, H0 = m.H[0], V = zs ? m.C : m.V, n_tiles = m.n_tiles;
    const int32_t *tstart = m.ws_tstart, *indices = m.indices, *nbp = m.ws_nb;
    const float *values = m.values, *dz0 = m.ws_dz[0];
    float* w_in = m.w_in + (ctxt && !zs ? (size_t)m.V * m.H[0] : 0);
    keep(B, H0, V, n_tiles, tstart, indices, nbp, values, dz0, w_in);
    const int H0P = rup(H0, 16);
    const int XS = stride_a(B), ZS = stride_b(H0P);
    float* xt = smem;
    float* dz = smem + 64 * XS;
    const int tile = ctxt ? rr : (int)gfk_bx(), c0 = tile * 64;

    GFK_STAMP(m, 40);
#ifdef GFK_STAMPS
    const bool stamp2 = m.n_batch > 1 && !ctxt && (tile == 0 || tile == n_tiles - 1);
    const int slot2 = tile == 0 ? 640 : 648;
#endif
    GFK_STAMP_IF(m, stamp2, slot2);
    // ---- staging: dz0 rows (zero padding), zero x^T tile, the tile's CSR extents ----
    const int nb = *nbp;
    if (H0P <= 64) {            // column tid % 64, rows tid / 64 + UT / 64 j: no runtime division
      const int c = tid & 63;
      if (c < H0P)
        for (int r = tid >> 6; r < B; r += UT / 64)
          dz[r * ZS + c] = (c < H0 && r < nb) ? dz0[r * H0 + c] : 0.f;
    } else {
      for (int i = tid; i < B * H0P; i += UT) {
        const int r = i / H0P, c = i % H0P;
        dz[r * ZS + c] = (c < H0 && r < nb) ? dz0[r * H0 + c] : 0.f;
      }
    }
    if (zs) {                   // x_ctx^T tile: the batch rows' contextual features
      for (int i = tid; i < B * 64; i += UT) {
        const int b = i >> 6, v = i & 63;
        xt[v * XS + b] = (b < nb && c0 + v < V) ? m.ctx[(size_t)m.ws_doc[b] * V + c0 + v] : 0.f;
      }
    } else if (ctxt) {          // A^T tile: the adapted rows (slab 0 of ctx_fwd's output)
      const float* ag = m.ws_actx + (size_t)tile * B * 64;
      for (int i = tid; i < B * 64; i += UT) {
        const int b = i >> 6, v = i & 63;
        xt[v * XS + b] = b < nb ? ag[i] : 0.f;
      }
    } else {
      for (int i = tid; i < 64 * XS; i += UT) xt[i] = 0.f;
    }
    // 16 threads per row: the row's non-zeros inside this tile (rows tid/16 + 32 i,
    // i < B / 32 -- the tile-start loads of every row are issued in the staging round)
    constexpr int XR = 128 / (UT / 16);          // row slots per thread (bmax <= 128)
    const int row = tid >> 4, sub = tid & 15;
    int xe0[XR], xe1[XR];
#pragma unroll
    for (int i = 0; i < XR; ++i) {
      const int r = row + i * (UT / 16);
      xe0[i] = xe1[i] = 0;
      if (!ctxt && r < nb && r < B) {
        const int32_t* ts = tstart + (size_t)r * (n_tiles + 1) + tile;
        xe0[i] = ts[0];
        xe1[i] = ts[1];
      }
    }
    GFK_STAMP_IF_VM(m, stamp2, slot2 + 1);
    // prefetch the optimizer state of this lane's outputs: subtiles t = wave + UW u
    // (16x16 each; H0 <= 64 -> at most 16 subtiles, one pass; wider layers take passes
    // of UW * PU subtiles below, the later ones prefetched after the scatter)
    const int MT = 4, NT = H0P / 16;
    constexpr int PU = 16 / UW;
    float pp[PU][4], pm[PU][4], pv[PU][4];
    const bool fused = m.update_mode == 1;
    // FLAT (H0 <= 64, one pass): a tile's W_in block [64, H0] is contiguous, so the
    // epilogue moves p / m / v as flat quads (float4 when 16-B aligned): every load /
    // store instruction covers whole cache lines, instead of the MFMA output layout's
    // 4 rows x 64 B.  The gradient tile goes through LDS (the x^T buffer, free after the
    // MFMAs).  Quad q of the block is thread (q % UT)'s slot q / UT.
    // (the 8-wave large-vocabulary shape only: with one round of 16-wave workgroups the
    // extra LDS pass and barriers measured slower than the bytes they save)
    const bool flat = UT == 512 && NT <= 4;
    const int nel = (min(V, c0 + 64) - c0) * H0;          // the block's elements
    float* wblk = w_in + (size_t)c0 * H0;
    const bool al4 = ((uintptr_t)wblk % 16 == 0) && m.off_m % 4 == 0 && m.off_v % 4 == 0 &&
                     m.off_g % 4 == 0;
    auto ld4 = [&](const float* q, int e) {      // elements e..e+3 of the block (bounded)
      if (al4 && e + 3 < nel) return *reinterpret_cast<const f32x4*>(q + e);
      f32x4 r;
#pragma unroll
      for (int i = 0; i < 4; ++i) r[i] = e + i < nel ? q[e + i] : 0.f;
      return r;
    };
    constexpr int FQ = 64 * 64 / 4 / UT;         // quads per thread (H0 <= 64)
    static_assert(FQ <= PU, "flat epilogue reuses the prefetch registers");
    if (flat) {
#pragma unroll
      for (int u = 0; u < FQ; ++u) {
        const int e = 4 * (tid + UT * u);
        f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = a, c = a;
        if (fused && e < nel) { a = ld4(wblk, e); b = ld4(wblk + m.off_m, e); c = ld4(wblk + m.off_v, e); }
#pragma unroll
        for (int i = 0; i < 4; ++i) { pp[u][i] = a[i]; pm[u][i] = b[i]; pv[u][i] = c[i]; }
      }
    }
#pragma unroll
    for (int u = 0; u < PU; ++u) {
      if (flat) break;
      const int t = wave + UW * u;
      const int i0 = (t / NT) * 16, j0 = (t % NT) * 16;
      const int j = min(j0 + (lane & 15), H0 - 1);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int v = min(c0 + i0 + (lane >> 4) * 4 + r, V - 1);
        float* p = w_in + (size_t)v * H0 + j;
        pp[u][r] = pm[u][r] = pv[u][r] = 0.f;
        if (t < MT * NT && fused) {
          pp[u][r] = *p;
          pm[u][r] = p[m.off_m];
          pv[u][r] = p[m.off_v];
        }
      }
    }
    __syncthreads();
    GFK_STAMP_IF(m, stamp2, slot2 + 2);
#pragma unroll
    for (int i = 0; i < XR; ++i) {
      const int r = row + i * (UT / 16);
      for (int e = xe0[i] + sub; e < xe1[i]; e += 16) xt[(indices[e] - c0) * XS + r] = values[e];
    }
    __syncthreads();

    GFK_STAMP(m, 41);
    GFK_STAMP_IF(m, stamp2, slot2 + 3);
    // ---- G[v, j] = sum_b xt[v, b] dz[b, j] and the update ----
    const AdamCoef ac = adam_coef(m);
    const bool sh = is_shared(m, w_in);
    f32x4 gk[PU];
    for (int pass = 0; pass * UW * PU < MT * NT; ++pass) {
    if (pass > 0) {             // wide input layers (H0 > 64): the next subtiles' state
#pragma unroll
      for (int u = 0; u < PU; ++u) {
        const int t = pass * UW * PU + wave + UW * u;
        const int i0 = (t / NT) * 16, j0 = (t % NT) * 16;
        const int j = min(j0 + (lane & 15), H0 - 1);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int v = min(c0 + i0 + (lane >> 4) * 4 + r, V - 1);
          float* p = w_in + (size_t)v * H0 + j;
          pp[u][r] = pm[u][r] = pv[u][r] = 0.f;
          if (t < MT * NT && fused) {
            pp[u][r] = *p;
            pm[u][r] = p[m.off_m];
            pv[u][r] = p[m.off_v];
          }
        }
      }
    }
#pragma unroll
    for (int u = 0; u < PU; ++u) {
      const int t = pass * UW * PU + wave + UW * u;
      if (t >= MT * NT) break;
      const int i0 = (t / NT) * 16, j0 = (t % NT) * 16;
      const float* ap = xt + (i0 + (lane & 15)) * XS + (lane >> 4);
      const float* bp = dz + (lane >> 4) * ZS + j0 + (lane & 15);
      f32x4 c0v = {0.f, 0.f, 0.f, 0.f}, c1v = {0.f, 0.f, 0.f, 0.f};
      for (int k = 0; k < B; k += 8) {
        c0v = mfma16x16x4(ap[k], bp[k * ZS], c0v);
        c1v = mfma16x16x4(ap[k + 4], bp[(k + 4) * ZS], c1v);
      }
      const f32x4 g = c0v + c1v;
      const int j = j0 + (lane & 15);
      if (flat) {               // park the gradient in registers until every wave is done
        gk[u] = g;
        continue;
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int v = c0 + i0 + (lane >> 4) * 4 + r;
        if (v >= V || j >= H0) continue;
        float* p = w_in + (size_t)v * H0 + j;
        if (!fused) {
          p[m.off_g] = g[r];
        } else {
          float mo = pm[u][r], vo = pv[u][r];
          float np = adam_update(pp[u][r], g[r], mo, vo, ac);
          if (sh && m.fed_scale_on) np *= m.fed_scale;
          p[m.off_m] = mo;
          p[m.off_v] = vo;
          p[gfk_own<GB>(m)] = np;
        }
      }
    }
    }
    if (flat) {
      // the gradient tile [64, H0] into x^T's buffer in the block's own (flat) order
      __syncthreads();
#pragma unroll
      for (int u = 0; u < PU; ++u) {
        const int t = wave + UW * u;
        if (t >= MT * NT) break;
        const int i0 = (t / NT) * 16, j0 = (t % NT) * 16, j = j0 + (lane & 15);
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (j < H0) xt[(i0 + (lane >> 4) * 4 + r) * H0 + j] = gk[u][r];
      }
      __syncthreads();
#pragma unroll
      for (int u = 0; u < FQ; ++u) {
        const int e = 4 * (tid + UT * u);
        if (e >= nel) break;
        const f32x4 g = *reinterpret_cast<const f32x4*>(xt + e);
        f32x4 np, mo, vo;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          float a = pm[u][i], b = pv[u][i];
          float x = fused ? adam_update(pp[u][i], g[i], a, b, ac) : g[i];
          np[i] = sh && m.fed_scale_on && fused ? x * m.fed_scale : x;
          mo[i] = a;
          vo[i] = b;
        }
        auto st4 = [&](float* q, const f32x4& x) {
          if (al4 && e + 3 < nel) { *reinterpret_cast<f32x4*>(q + e) = x; return; }
#pragma unroll
          for (int i = 0; i < 4; ++i) if (e + i < nel) q[e + i] = x[i];
        };
        if (!fused) {
          st4(wblk + m.off_g, np);
        } else {
          st4(wblk + m.off_m, mo);
          st4(wblk + m.off_v, vo);
          st4(wblk + gfk_own<GB>(m), np);
        }
      }
    }
    GFK_STAMP(m, 42);
    GFK_STAMP_IF_VM(m, stamp2, slot2 + 4);
  } else {
  // ---- the 6-waves-per-SIMD instance: the staging as ONE global round (it holds the round's
  //      loads in registers the 64-VGPR instances do not have: there it measured slower) ----
    const bool zs = m.ctx_fused == 2;            // ZeroShotTM: W_in is the dense [C, H0] layer
    if (m.input == GFK_IN_CONTEXTUAL && !zs) return;   // (host GEMMs when not fused)
    const int rr = (int)gfk_bx() - (nt_here + U.n_w + U.n_v + 1);
    const bool ctxt = rr >= 0;                   // a Wc tile (CombinedTM) / W tile (ZeroShotTM)
    if (zs && !ctxt) return;                     // ZeroShotTM has no bag-of-words half
    const int tid = threadIdx.x, lane = tid & 63, wave = uniform(tid >> 6);
    int B = m.bmax, H0 = m.H[0], V = zs ? m.C : m.V, n_tiles = m.n_tiles;
    // (global address space: the batched descriptor's pointers are generic, and one pending
    // FLAT load turns every later wait into vmcnt(0) lgkmcnt(0) -- no load could stay in flight)
    typedef const __attribute__((address_space(1))) int32_t* gci_t;
    typedef const __attribute__((address_space(1))) float* gcf_t;
    typedef __attribute__((address_space(1))) float* gf_t;
    typedef __attribute__((address_space(1))) f32x4* gq_t;
    // element at a 32-bit BYTE offset from a uniform base: the offset stays one VGPR (the scalar
    // base + 32-bit offset form of the load), not a 64-bit address pair per load in flight
    auto at32 = [](auto base, unsigned byte_off) {
      typedef __attribute__((address_space(1))) char* gch_t;
      return *(decltype(base))((gch_t)base + byte_off);
    };
    gci_t tstart = (gci_t)m.ws_tstart, indices = (gci_t)m.indices, nbp = (gci_t)m.ws_nb;
    gcf_t values = (gcf_t)m.values, dz0 = (gcf_t)m.ws_dz[0];
    const float* w_in_flat = m.w_in + (ctxt && !zs ? (size_t)m.V * m.H[0] : 0);
    gf_t w_in = (gf_t)w_in_flat;
    keep(B, H0, V, n_tiles, tstart, indices, nbp, values, dz0, w_in);
    const int H0P = rup(H0, 16);
    const int XS = stride_a(B), ZS = stride_b(H0P);
    float* xt = smem;
    float* dz = smem + 64 * XS;
    const int tile = ctxt ? rr : (int)gfk_bx(), c0 = tile * 64;
    const int MT = 4, NT = H0P / 16;
    const bool fused = m.update_mode == 1;
    const int nel = (min(V, c0 + 64) - c0) * H0;          // the block's elements
    gf_t wblk = w_in + (size_t)c0 * H0;
    const bool al4 = ((uintptr_t)wblk % 16 == 0) && m.off_m % 4 == 0 && m.off_v % 4 == 0 &&
                     m.off_g % 4 == 0;
    // FLAT (H0 <= 64, one pass): a tile's W_in block [64, H0] is contiguous, so the
    // epilogue moves p / m / v as flat quads (whole float4: 16-B aligned blocks of a multiple
    // of 4 elements; other blocks take the subtile layout): every load / store instruction
    // covers whole cache lines, instead of the MFMA output layout's 4 rows x 64 B.  The
    // gradient tile goes through LDS (the x^T buffer, free after the MFMAs).  Quad q of the
    // block is thread (q % UT)'s slot q / UT.
    // (the 8-wave large-vocabulary shape only: with one round of 16-wave workgroups the
    // extra LDS pass and barriers measured slower than the bytes they save)
    // The tile body is compiled once per layout (a compile-time `flat`): the flat prefetch is
    // then straight-line code, and a load issued in it can stay in flight -- behind a
    // run-time branch the compiler's wait-count pass merges the paths and waits for everything.
    const bool flat_rt = uniform(UT == 512 && NT <= 4 && al4 && nel % 4 == 0 && nel >= 4) != 0;

    GFK_STAMP_WG(m, !ctxt && tile == 0, 40);
    // batched launches: the first-tile and the last-tile workgroup, slots 640 / 648 + entry,
    // tile extents landed, first barrier passed, scatter done, end
#ifdef GFK_STAMPS
    const bool stamp2 = m.n_batch > 1 && !ctxt && (tile == 0 || tile == n_tiles - 1);
    const int slot2 = tile == 0 ? 640 : 648;
#endif
    GFK_STAMP_IF(m, stamp2, slot2);
    // ---- staging, one global round: every load whose address needs no other load is issued
    //      before the first wait.  Issue order matters (vmcnt counts in order): the rows' tile
    //      extents first, so the dependent first-non-zero loads wait for them alone while
    //      dz0 and the block's p / m / v stay in flight ----
    const int nb = *nbp;
    if (H0P > 64) {             // wide layers: dz0 staged ahead of the round (its guarded loads in
      for (int i = tid; i < B * H0P; i += UT) {   // a loop would make every later wait a full one)
        const int r = i / H0P, c = i % H0P;
        dz[r * ZS + c] = (c < H0 && r < nb) ? dz0[r * H0 + c] : 0.f;
      }
    }
    // 16 threads per row: the row's non-zeros inside this tile (rows tid/16 + 32 i,
    // i < B / 32).  Unconditional loads of clamped rows (the table has bmax rows; a contextual
    // tile reads column 0 and drops it): behind `r < nb` they would wait for nb's round trip
    constexpr int XR = 128 / (UT / 16);          // row slots per thread (bmax <= 128)
    const int row = tid >> 4, sub = tid & 15;
    int xe0[XR], xe1[XR];
#pragma unroll
    for (int i = 0; i < XR; ++i) {
      const int r = min(row + i * (UT / 16), B - 1);
      const unsigned ts = 4u * (unsigned)(r * (n_tiles + 1) + (ctxt ? 0 : tile));   // (bytes: 4 B n_tiles)
      xe0[i] = at32(tstart, ts);
      xe1[i] = at32(tstart, ts + 4u);
    }
    __builtin_amdgcn_sched_barrier(0);
    // dz0 rows tid / 64 + UW u, column tid % 64 (H0P <= 64; no runtime division): clamped,
    // unconditional (wider layers drop them: no branch between the loads of this round),
    // DZU rows per thread in flight (128 rows at 8 waves: two chunks)
    constexpr int DZU = 8;
    const int zc = tid & 63;
    float dzr[DZU];
    auto dz_issue = [&](int r0) {
#pragma unroll
      for (int u = 0; u < DZU; ++u) {
        const int r = min(r0 + (tid >> 6) + UW * u, B - 1);
        dzr[u] = at32(dz0, 4u * (unsigned)(r * H0 + min(zc, H0 - 1)));
      }
    };
    auto dz_store = [&](int r0) {
#pragma unroll
      for (int u = 0; u < DZU; ++u) {
        // an integer mask, not a select (a select lets the compiler sink the load into a
        // branch + vmcnt(0) each; 0 * x would keep a NaN of the rows past nb)
        // (the value is waited for by every lane, ahead of the guarded store: a wait inside
        // the branch leaves the load "maybe pending" for the wait-count pass on the other path)
        const int r = r0 + (tid >> 6) + UW * u;
        const unsigned keepm = (zc < H0 && r < nb) ? ~0u : 0u;
        asm volatile("" : "+v"(dzr[u]));
        if (zc < H0P && r < B) dz[r * ZS + zc] = __uint_as_float(__float_as_uint(dzr[u]) & keepm);
      }
    };
    dz_issue(0);
    __builtin_amdgcn_sched_barrier(0);
    // rows >= nb carry an earlier batch's extents (or none): masked AFTER the load, so nothing
    // behind a dead row is dereferenced; then each row slot's first (index, value) pair,
    // clamped into the row's extent (an empty extent reads a neighbouring entry and drops it)
    int xc[XR];
    float xv[XR];
#pragma unroll
    for (int i = 0; i < XR; ++i) {
      const int r = row + i * (UT / 16);
      const int live = (!ctxt && r < nb && r < B) ? -1 : 0;
      xe0[i] &= live;
      xe1[i] &= live;
    }
#pragma unroll
    for (int i = 0; i < XR; ++i) {               // (a contextual tile reads entry 0 and drops it)
      const unsigned e = (unsigned)min(xe0[i] + sub, max(xe1[i] - 1, 0));
      xc[i] = indices[e];
      xv[i] = values[e];
    }
    __builtin_amdgcn_sched_barrier(0);
    GFK_STAMP_IF(m, stamp2, slot2 + 1);
    // ---- LDS: dz0 rows (zero padding).  Ahead of the p / m / v prefetch: it waits for dz0
    //      alone (the first-non-zero pairs behind it stay in flight) and frees its registers
    //      before the prefetch takes 24 -- the prefetch starts one L2 round trip later ----
    if (H0P <= 64) {
      dz_store(0);
      for (int r0 = DZU * UW; r0 < B; r0 += DZU * UW) {
        dz_issue(r0);
        dz_store(r0);
      }
    }
    // (the round's loads so far are common to both layouts and issued once, ahead of the split)
    auto body = [&](auto flat_c) {
    constexpr bool flat = decltype(flat_c)::value;
    // prefetch the optimizer state of this lane's outputs: subtiles t = wave + UW u
    // (16x16 each; H0 <= 64 -> at most 16 subtiles, one pass; wider layers take passes
    // of UW * PU subtiles below, the later ones prefetched after the scatter)
    constexpr int PU = 16 / UW;
    float pp[PU][4], pm[PU][4], pv[PU][4];
    constexpr int FQ = 64 * 64 / 4 / UT;         // quads per thread (H0 <= 64)
    static_assert(FQ <= PU, "flat epilogue reuses the prefetch registers");
    if (flat) {
      // unconditional, clamped quads (threads past the block re-read its last quad and drop
      // it; gradient mode reads the parameter three times): no select on a pending load
      const int64_t om = fused ? m.off_m : 0, ov = fused ? m.off_v : 0;
#pragma unroll
      for (int u = 0; u < FQ; ++u) {
        const unsigned e = 4u * (unsigned)min(4 * (tid + UT * u), nel - 4);      // (bytes: <= 16 KiB)
        const f32x4 a = at32((gq_t)wblk, e), b = at32((gq_t)(wblk + om), e), c = at32((gq_t)(wblk + ov), e);
#pragma unroll
        for (int i = 0; i < 4; ++i) { pp[u][i] = a[i]; pm[u][i] = b[i]; pv[u][i] = c[i]; }
      }
    }
#pragma unroll
    for (int u = 0; u < PU; ++u) {
      if (flat) break;
      const int t = wave + UW * u;
      const int i0 = (t / NT) * 16, j0 = (t % NT) * 16;
      const int j = min(j0 + (lane & 15), H0 - 1);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int v = min(c0 + i0 + (lane >> 4) * 4 + r, V - 1);
        gf_t p = w_in + (size_t)v * H0 + j;
        pp[u][r] = pm[u][r] = pv[u][r] = 0.f;
        if (t < MT * NT && fused) {
          pp[u][r] = *p;
          pm[u][r] = p[m.off_m];
          pv[u][r] = p[m.off_v];
        }
      }
    }
    // ---- LDS: the x^T tile zeroed (contextual tiles: filled) ----
    if (zs) {                   // x_ctx^T tile: the batch rows' contextual features
      for (int i = tid; i < B * 64; i += UT) {
        const int b = i >> 6, v = i & 63;
        xt[v * XS + b] = (b < nb && c0 + v < V) ? m.ctx[(size_t)m.ws_doc[b] * V + c0 + v] : 0.f;
      }
    } else if (ctxt) {          // A^T tile: the adapted rows (slab 0 of ctx_fwd's output)
      const float* ag = m.ws_actx + (size_t)tile * B * 64;
      for (int i = tid; i < B * 64; i += UT) {
        const int b = i >> 6, v = i & 63;
        xt[v * XS + b] = b < nb ? ag[i] : 0.f;
      }
    } else {
      for (int i = tid; i < 64 * XS; i += UT) xt[i] = 0.f;
    }
    // (staged global data reaches LDS through registers, whose loads the compiler waits for:
    // both barriers order LDS traffic only, and p / m / v stay in flight across them)
    lds_barrier();              // the zero fill is done before the scatter
    GFK_STAMP_IF(m, stamp2, slot2 + 2);
#pragma unroll
    for (int i = 0; i < XR; ++i) asm volatile("" : "+v"(xc[i]), "+v"(xv[i]));   // (as for dz0 above)
#pragma unroll
    for (int i = 0; i < XR; ++i) {
      const int r = row + i * (UT / 16);
      // the preloaded pair is the row slot's first entry; a tile holds more than 16
      // non-zeros of a row rarely (~2 per row per tile at V = 4.7k)
      for (int k = 0, e = xe0[i] + sub; e < xe1[i]; ++k, e += 16) {
        const int c = (k == 0 ? xc[i] : indices[e]) - c0;
        xt[c * XS + r] = k == 0 ? xv[i] : values[e];
      }
    }
    lds_barrier();

    GFK_STAMP_WG(m, !ctxt && tile == 0, 41);
    GFK_STAMP_IF(m, stamp2, slot2 + 3);
    // ---- G[v, j] = sum_b xt[v, b] dz[b, j] and the update ----
    const AdamCoef ac = adam_coef(m);
    const bool sh = is_shared(m, w_in_flat);
    f32x4 gk[PU];
    for (int pass = 0; pass * UW * PU < MT * NT; ++pass) {
    if (pass > 0) {             // wide input layers (H0 > 64): the next subtiles' state
#pragma unroll
      for (int u = 0; u < PU; ++u) {
        const int t = pass * UW * PU + wave + UW * u;
        const int i0 = (t / NT) * 16, j0 = (t % NT) * 16;
        const int j = min(j0 + (lane & 15), H0 - 1);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int v = min(c0 + i0 + (lane >> 4) * 4 + r, V - 1);
          gf_t p = w_in + (size_t)v * H0 + j;
          pp[u][r] = pm[u][r] = pv[u][r] = 0.f;
          if (t < MT * NT && fused) {
            pp[u][r] = *p;
            pm[u][r] = p[m.off_m];
            pv[u][r] = p[m.off_v];
          }
        }
      }
    }
#pragma unroll
    for (int u = 0; u < PU; ++u) {
      const int t = pass * UW * PU + wave + UW * u;
      if (t >= MT * NT) break;
      const int i0 = (t / NT) * 16, j0 = (t % NT) * 16;
      const float* ap = xt + (i0 + (lane & 15)) * XS + (lane >> 4);
      const float* bp = dz + (lane >> 4) * ZS + j0 + (lane & 15);
      f32x4 c0v = {0.f, 0.f, 0.f, 0.f}, c1v = {0.f, 0.f, 0.f, 0.f};
      for (int k = 0; k < B; k += 8) {
        c0v = mfma16x16x4(ap[k], bp[k * ZS], c0v);
        c1v = mfma16x16x4(ap[k + 4], bp[(k + 4) * ZS], c1v);
      }
      const f32x4 g = c0v + c1v;
      const int j = j0 + (lane & 15);
      if (flat) {               // park the gradient in registers until every wave is done
        gk[u] = g;
        continue;
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int v = c0 + i0 + (lane >> 4) * 4 + r;
        if (v >= V || j >= H0) continue;
        gf_t p = w_in + (size_t)v * H0 + j;
        if (!fused) {
          p[m.off_g] = g[r];
        } else {
          float mo = pm[u][r], vo = pv[u][r];
          float np = adam_update(pp[u][r], g[r], mo, vo, ac);
          if (sh && m.fed_scale_on) np *= m.fed_scale;
          p[m.off_m] = mo;
          p[m.off_v] = vo;
          p[gfk_own<GB>(m)] = np;
        }
      }
    }
    }
    if (flat) {
      // the gradient tile [64, H0] into x^T's buffer in the block's own (flat) order
      __syncthreads();
#pragma unroll
      for (int u = 0; u < PU; ++u) {
        const int t = wave + UW * u;
        if (t >= MT * NT) break;
        const int i0 = (t / NT) * 16, j0 = (t % NT) * 16, j = j0 + (lane & 15);
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (j < H0) xt[(i0 + (lane >> 4) * 4 + r) * H0 + j] = gk[u][r];
      }
      __syncthreads();
#pragma unroll
      for (int u = 0; u < FQ; ++u) {
        const int e = 4 * (tid + UT * u);
        if (e >= nel) break;
        const f32x4 g = *reinterpret_cast<const f32x4*>(xt + e);
        f32x4 np, mo, vo;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          float a = pm[u][i], b = pv[u][i];
          float x = fused ? adam_update(pp[u][i], g[i], a, b, ac) : g[i];
          np[i] = sh && m.fed_scale_on && fused ? x * m.fed_scale : x;
          mo[i] = a;
          vo[i] = b;
        }
        auto st4 = [&](gf_t q, const f32x4& x) {
          if (al4 && e + 3 < nel) { *(gq_t)(q + e) = x; return; }
#pragma unroll
          for (int i = 0; i < 4; ++i) if (e + i < nel) q[e + i] = x[i];
        };
        if (!fused) {
          st4(wblk + m.off_g, np);
        } else {
          st4(wblk + m.off_m, mo);
          st4(wblk + m.off_v, vo);
          st4(wblk + gfk_own<GB>(m), np);
        }
      }
    }
    GFK_STAMP_WG(m, !ctxt && tile == 0, 42);
    GFK_STAMP_IF_VM(m, stamp2, slot2 + 4);
    };
    // (the subtile layout ends the kernel in its own branch: nothing of it is pending where the
    // flat layout starts)
    if (!flat_rt) {
      body(std::false_type{});
      return;
    }
    body(std::true_type{});
  }
}

// The large-batch plan's dense W_in tile (bmax > 128, gradient mode, H0 <= 64): the W_in
// tile body above with the batch taken in chunks of 128 rows -- per chunk the x^T tile
// [64][130] is rebuilt from the chunk rows' tile extents and dz0's chunk [128][ZS] staged,
// the MFMA accumulators carrying over (the small vocabularies' dense tiles: at V = 4.5k
// a 64-word tile holds ~700 of a 256-row batch's non-zeros, which the entry-list walk of the
// sparse tile serialises).  LDS: 64 x 130 + 128 x stride_b(H0) floats.
template <int UT>
__device__ __forceinline__ void win_tile_dense_ch(const GfkModel& m, float* smem, int tile) {
  constexpr int UW = UT / 64, RC = WJ_ROWS;
  constexpr int PU = 16 / UW;                  // subtiles per wave (H0 <= 64: 16 in all)
  constexpr int XR = RC / (UT / 16);           // row slots per thread per chunk
  const int tid = threadIdx.x, lane = tid & 63, wave = uniform(tid >> 6);
  const int B = m.bmax, H0 = m.H[0], V = m.V, n_tiles = m.n_tiles, c0 = tile * 64;
  const int nb = *m.ws_nb;
  const int H0P = rup(H0, 16), NT = H0P / 16, MT = 4;
  const int XS = stride_a(RC), ZS = stride_b(H0P);
  float* xt = smem;
  float* dz = smem + 64 * XS;
  const float* dz0 = m.ws_dz[0];
  const int row = tid >> 4, sub = tid & 15;
  f32x4 g[PU];
#pragma unroll
  for (int u = 0; u < PU; ++u) g[u] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int b0 = 0; b0 < B; b0 += RC) {
    if (b0) __syncthreads();                   // the previous chunk's operand reads are done
    {
      const int c = tid & 63;
      if (c < H0P)
        for (int r = tid >> 6; r < RC; r += UT / 64)
          dz[r * ZS + c] = (c < H0 && b0 + r < nb) ? dz0[(size_t)(b0 + r) * H0 + c] : 0.f;
    }
    for (int i = tid; i < 64 * XS; i += UT) xt[i] = 0.f;
    int xe0[XR], xe1[XR];
#pragma unroll
    for (int i = 0; i < XR; ++i) {
      const int r = b0 + row + i * (UT / 16);
      xe0[i] = xe1[i] = 0;
      if (r < nb) {
        const int32_t* ts = m.ws_tstart + (size_t)r * (n_tiles + 1) + tile;
        xe0[i] = ts[0];
        xe1[i] = ts[1];
      }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < XR; ++i) {
      const int rl = row + i * (UT / 16);
      for (int e = xe0[i] + sub; e < xe1[i]; e += 16) xt[(m.indices[e] - c0) * XS + rl] = m.values[e];
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < PU; ++u) {
      const int t = wave + UW * u;
      if (t >= MT * NT) break;
      const int i0 = (t / NT) * 16, j0 = (t % NT) * 16;
      const float* ap = xt + (i0 + (lane & 15)) * XS + (lane >> 4);
      const float* bp = dz + (lane >> 4) * ZS + j0 + (lane & 15);
      f32x4 c0v = {0.f, 0.f, 0.f, 0.f}, c1v = {0.f, 0.f, 0.f, 0.f};
      for (int k = 0; k < RC; k += 8) {
        c0v = mfma16x16x4(ap[k], bp[k * ZS], c0v);
        c1v = mfma16x16x4(ap[k + 4], bp[(k + 4) * ZS], c1v);
      }
      g[u] += c0v + c1v;
    }
  }
  float* w_in = m.w_in;
#pragma unroll
  for (int u = 0; u < PU; ++u) {
    const int t = wave + UW * u;
    if (t >= MT * NT) break;
    const int i0 = (t / NT) * 16, j = (t % NT) * 16 + (lane & 15);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int v = c0 + i0 + (lane >> 4) * 4 + r;
      if (v < V && j < H0) w_in[(size_t)v * H0 + j + m.off_g] = g[u][r];
    }
  }
}

// the large-batch plan's update kernel with dense W_in tiles: job workgroups first, then the
// n_tiles chunked tiles
template <int UT>
__global__ void __launch_bounds__(UT) gfk_win_lb_k(GfkArgT<false> ga, GfkUArgT<false> gua) {
  const GfkModel& m = ga.m;
  const GfkUpdate& U = gua.u;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int r = (int)blockIdx.x;
  if (r < U.n_w) { weight_job_lb<UT>(m, U.w[r], smem); return; }
  if (r < U.n_w + U.n_v) { vector_job<UT, true>(m, U.v[r - U.n_w]); return; }
  if (r == U.n_w + U.n_v) { prepare_next_batch(m, reinterpret_cast<int*>(smem)); return; }
  win_tile_dense_ch<UT>(m, smem, r - (U.n_w + U.n_v + 1));
}

// the sparse W_in tiles (stage_flags bit 4) as their own kernel: its register budget is
// its own (the job paths of gfk_win_update_k need ~86 VGPRs)
// grid: n_w + n_v + 1 job workgroups FIRST (they start with the tiles, not after them),
// then the n_tiles sparse W_in tiles (+ n_tiles dense contextual tiles: fused CombinedTM)
template <int UT, bool GB = false, bool VL = false, bool CTX = false, int RS = 2>
__global__ void __launch_bounds__(UT, VL ? 4096 / UT : 1) gfk_win_sparse_k(GfkArgT<GB> ga, GfkUArgT<GB> gua) {
  const GfkModel& m = gfk_model(ga);
  const GfkUpdate& U = gfk_upd(gua);
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int r = (int)gfk_bx();
  if (r < U.n_w) {
    if constexpr (RS > 2) weight_job_lb<UT>(m, U.w[r], smem);
    else weight_job<UT, GB>(m, U.w[r], smem);
    return;
  }
  if (r < U.n_w + U.n_v) { vector_job<UT, (RS > 2), GB>(m, U.v[r - U.n_w]); return; }
  if (r == U.n_w + U.n_v) { prepare_next_batch(m, reinterpret_cast<int*>(smem)); return; }
  const int t = r - (U.n_w + U.n_v + 1);
  if constexpr (CTX) {
    if (t >= m.n_tiles) { win_tile_ctx<UT>(m, smem, t - m.n_tiles); return; }
  }
  win_tile_sparse<UT, VL, RS, GB>(m, smem, t);
}

// the sparse tile's LDS second-moment variant: fused mode, and the block fits the LDS the
// kernel is given anyway (gfk_win_update_smem: no occupancy lost to LDS); gradient mode and
// the large-batch plan keep the second moment in registers
static bool win_sparse_vl(const GfkModel* m) {
  if (m->update_mode != 1) return false;
  if (m->bmax > 128) return false;      // (the large-batch instance keeps it in registers)
  const size_t need = sizeof(float) * ((((size_t)m->bmax * m->H[0] + 2 * 512 + 129 + 3) & ~(size_t)3) +
                                       (size_t)64 * m->H[0]);
  return need <= gfk_win_update_smem(m);
}

// The instance table (csrc/gfk_launch.h): the launcher looks its kernel up by the key it
// computes from the model, and gfk_win_update_set_smem raises the dynamic-LDS limit of the
// same rows.  A new instance is one new row.
// {kernel, threads, waves per SIMD where not the shape's own} the dense tiles | {kernel, LDS second moment, contextual tiles, large batch}
// the sparse tiles | {kernel} the large-batch chunked dense tiles (one client)
enum { WINK_DENSE, WINK_SPARSE, WINK_LB };
#define WIN_SPARSE_ROW(VL, CTX) {{WINK_SPARSE, VL, CTX}, {gfk_win_sparse_k<512, false, VL, CTX>, gfk_win_sparse_k<512, true, VL, CTX>}}
static const GfkRowU kWinUpdate[] = {
    {{WINK_DENSE, 512}, GFK_PAIR(gfk_win_update_k, 512)},
    {{WINK_DENSE, 1024}, GFK_PAIR(gfk_win_update_k, 1024)},
    {{WINK_DENSE, 512, 6}, {nullptr, gfk_win_update_k<512, true, 6>}},
    WIN_SPARSE_ROW(false, false), WIN_SPARSE_ROW(true, false), WIN_SPARSE_ROW(false, true), WIN_SPARSE_ROW(true, true),
    {{WINK_SPARSE, 0, 0, 1}, {gfk_win_sparse_k<512, false, false, false, GFK_BMAX_LIMIT / 64>,
                              gfk_win_sparse_k<512, true, false, false, GFK_BMAX_LIMIT / 64>}},
    {{WINK_LB}, {gfk_win_lb_k<1024>, nullptr}}};
#undef WIN_SPARSE_ROW

extern "C" int gfk_launch_win_update(const GfkModel* m, const GfkUpdate* u, hipStream_t s) {
  const int extra = m->ctx_fused == 1 ? m->n_tiles : (m->ctx_fused == 2 ? (m->C + 63) / 64 : 0);
  const size_t sm = gfk_win_update_smem(m);
  if (m->stage_flags & WIN_SPARSE) {
    // bag-of-words inputs, or fused CombinedTM (its contextual half as dense tiles after
    // the sparse ones: B <= 64 so the operand blocks fit the kernel's LDS)
    const bool comb = m->input == GFK_IN_COMBINED && m->ctx_fused == 1;
    if (m->H[0] > 64 || m->bmax > (comb ? 64 : GFK_BMAX_LIMIT) || !(m->input == GFK_IN_BOW || comb))
      return -1;
    const dim3 gs(u->n_w + u->n_v + 1 + m->n_tiles * (comb ? 2 : 1));
    // (the large-batch instance: never with the LDS second moment -- win_sparse_vl -- nor
    // with contextual tiles -- comb: B <= 64)
    return gfk_launch(gfk_find(kWinUpdate, WINK_SPARSE, win_sparse_vl(m), comb, m->bmax > 128), m, u, gs,
                      dim3(512), sm, s);
  }
  if (m->bmax > 128) {                 // large batches: the chunked dense tiles
    if (m->H[0] > 64 || m->update_mode != 0 || m->input != GFK_IN_BOW || m->n_batch > 1) return -1;
    const dim3 gl(u->n_w + u->n_v + 1 + m->n_tiles);
    return gfk_launch(gfk_find(kWinUpdate, WINK_LB), m, u, gl, dim3(1024), sm, s);
  }
  const dim3 g(m->n_tiles + u->n_w + u->n_v + 1 + extra);
  // more W_in tiles than two rounds of 16-wave workgroups (dec_grid = the CUs' slots), or the
  // batched launch of several clients' tiles asks for the 8-wave shape (stage_flags bit 9,
  // set by BatchedSteps when all clients' tiles together exceed two rounds)
  const int nt = ((m->n_tiles > 2 * m->dec_grid && m->n_tiles > 512) || (m->stage_flags & WIN_BATCH8)) ? 512 : 1024;
  // (stage_flags GFK_WIN_WAVES6 asks for the 6-waves-per-SIMD instance of the 8-wave shape: a
  // launch it has no instance for is an error, never the other instance)
  const int wps = (m->stage_flags & GFK_WIN_WAVES6) ? 6 : 0;
  if (wps && nt != 512) return -1;
  return gfk_launch(gfk_find(kWinUpdate, WINK_DENSE, nt, wps), m, u, g, dim3(nt), sm, s);
}

extern "C" int gfk_win_update_set_smem(size_t bytes) {
  static size_t cur = 0;
  return gfk_lds_raised(cur, bytes) ? gfk_raise_lds(kWinUpdate, bytes) : 0;
}
