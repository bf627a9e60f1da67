// ProdLDA decoder: word_dist = softmax_V(BN_batch(theta_d @ beta)), its
// reconstruction loss -sum x log(word_dist + 1e-10), and the backward.
//
// Reference math: decoder_network.py:121-126, avitm.py:225.
//
// Tiling (MI355X-first): one workgroup (4 waves) owns one vocabulary tile of
// VB=64 columns x ALL batch rows (B <= 128), so the per-column batch-norm
// statistics (a reduction over B) never leave the workgroup, and the softmax
// over V is a per-row sum of exp (no max shift: BN bounds |z|) whose partials are merged by
// row_loss.  The three GEMM-shaped products run on the fp32 matrix cores
// (v_mfma_f32_16x16x4_f32, exact fp32 -- the reference is fp32):
//     logits[B, VB]  = theta_d[B, K] @ beta[K, VB]           (forward)
//     dbeta[K, VB]   = theta_d^T[K, B] @ dlogit[B, VB]       (backward, per tile)
//     dtheta_d[B, K] = sum_tiles dlogit[B, VB] @ beta^T[VB, K] (per-tile partials)
//
// Latency discipline (the kernels are tiny, so round trips dominate):
//  * every global read of a kernel is issued in ONE staging round before the
//    first barrier: theta_d and the BN'ed logit tile go through LDS-DMA
//    (global_load_lds_dwordx4), the beta tile through registers;
//  * forward: wave w owns columns [16w, 16w+16) for all rows, so the column
//    batch-norm statistics, the normalisation, the running-stat update and the
//    per-row sum-exp partials are computed straight from the MFMA
//    accumulators (cross-lane shuffles, no LDS pass, no second barrier);
//  * backward: the x tile is never materialised -- the sparse -x p/(p+1e-10)
//    terms are written into a pre-zeroed dlogit tile, then one register pass
//    adds p*S and applies the BN backward.
//
// The loss never needs the dense [B, V] word distribution: only the CSR
// non-zeros are gathered (row_loss), and the backward needs per row
//   dL/dz_bj = p_bj * S_b - x_bj * p_bj / (p_bj + 1e-10),
//   S_b = sum_{v in nz(b)} x_bv p_bv / (p_bv + 1e-10),
// with p recomputed from the stored BN'ed logits.  row_loss also records where
// each row's non-zeros of every vocab tile start (ws_tstart).
//
// Layouts: ws_thetad is [bmax, kt] (kt = K padded to 4 x odd, zero padding, so
// the MFMA A-operand reads are bank-conflict free); ws_zn is tiled
// [n_tiles][bmax][VB] so a tile is one contiguous LDS-DMA copy; ws_row_part is
// [dec_grid * 4][bmax][2] (one partial per forward wave column strip).
#define GFK_BATCHED_COPY 1   // batched kernels copy their descriptor (gfk_common.h gfk_model)
#include "gfk_common.h"
#include "gfk_launch.h"

using namespace gfk;

namespace {
constexpr int DEC_THREADS = 1024;
constexpr int VB = 64;
constexpr int LDB_F = 80;   // fwd beta tile stride: B-role reads (lane -> column) conflict free
// bwd strides, 2 mod 32: the transposed B-role reads of the beta tile (lane -> k row) and
// the A-role reads of dlogit (lane -> row) put 16 rows x 2 columns of a half-wave on 32
// distinct ds_read_b32 banks; so do the dense pass's 16 rows x 2 columns of dlogit
constexpr int LDB_B = 66;
constexpr int LDD = 66;
// BN'ed logit tiles (ws_zn) are stored XOR-swizzled: element (row, col) of a tile at
// row * VB + (col ^ zswz(row)).  The bwd dense pass reads 16 rows x 2 columns per
// half-wave; unswizzled (stride VB = 64) those 16 rows hit ONE bank (16-way conflict),
// swizzled they cover 32 distinct banks.  The tile is LDS-DMA'd verbatim, so the
// swizzle is applied by the writer (prodlda_fwd) and every reader.
__host__ __device__ __forceinline__ int zswz(int row) { return (row & 15) << 1; }
constexpr float RL_EPS = 1e-10f;

__host__ __device__ __forceinline__ int round_up(int x, int m) { return (x + m - 1) / m * m; }
// byte offset sum for buffer voffsets: unsigned (wrapping) arithmetic, since an out-of-range
// marker (0x7FFF0000) plus a row / column offset exceeds INT_MAX
__device__ __forceinline__ int boff(int a, int b) { return (int)((unsigned)a + (unsigned)b); }

// sum over the 4 lane groups (lanes l, l^16, l^32, l^48): a column reduction
__device__ __forceinline__ float sum_groups(float v) {
  v += __shfl_xor(v, 16, 64);
  v += __shfl_xor(v, 32, 64);
  return v;
}
}  // namespace

// grid: dec_grid workgroups of 16 waves (persistent: workgroup g owns vocab tiles
// g, g + dec_grid, ...; the usual case is one tile each).  theta_d is staged once per
// workgroup, so large vocabularies do not re-read it per tile, and the per-row
// sum-exp partials are accumulated across the workgroup's tiles in registers
// (ws_row_part holds dec_grid * 4 partials per row).  Wave w owns column strip
// cs = w & 3 (16 columns) and row tiles rt = (w >> 2) + 4 i.
// Several tiles per workgroup (large V): the next tile's beta block and running
// statistics are loaded into registers right after this tile's staging barrier, so
// they land while this tile's MFMAs / batch-norm / stores run.
// dynamic LDS: th[BM*kt] + bt[KP*LDB_F] + colp[4][64] + colq[4][64] + stat[2][64]
// BF: bf16 MFMA operands (16x16x32, a 16x16x16 tail; K padded to 16), fp32 accumulation.
template <int BM, bool BF, bool GB = false>
__global__ void __launch_bounds__(DEC_THREADS) prodlda_fwd_kernel(GfkArgT<GB> ga) {
  const GfkModel& m = gfk_model(ga);
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int K = m.K, V = m.V, KT = m.kt;
  int tid = threadIdx.x;                      // re-made opaque per tile (no hoisted addresses)
  const int lane = tid & 63, wave = uniform(tid >> 6);
  const int KP = round_up(K, BF ? 16 : 4);
  float* th = smem;
  float* bt = th + BM * KT;
  float* colp = bt + KP * LDB_F;
  float* colq = colp + 4 * VB;
  constexpr int RT = BM / 16;                 // row tiles
  constexpr int NRT = (RT + 3) / 4;           // row tiles per wave
  constexpr int BU = 16;                      // beta tile elements per thread (K <= 256)
  const int cs = wave & 3, rt0 = wave >> 2;
  const int col = 16 * cs + (lane & 15);      // this lane's column within a tile
  // this lane's running sum of exp(z) over its columns of every tile, per row.  No max
  // shift is needed: z is batch-normalised with the batch's own statistics, so
  // |z| <= sqrt(nb - 1) <= sqrt(127) (Samuelson) and exp(z) <= 8e4 -- the sum over any
  // vocabulary stays far inside fp32.  The 16 column lanes of a row are reduced once,
  // after the last tile, not per tile.
  float rs_[NRT][4];
#pragma unroll
  for (int i = 0; i < NRT; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) rs_[i][e] = 0.f;

  GFK_STAMP(m, 16);
  glds_copy(th, m.ws_thetad, BM * KT, tid, DEC_THREADS);
  const int nb = *m.ws_nb;
  if (gfk_bx() == 0 && tid == 0) *m.nbt_beta += 1;
  // a tile's beta block [0, KP) x [c0, c0 + VB) and running statistics, into registers
  float br[BU], rmr = 0.f, rvr = 0.f;
  // element tid + DEC_THREADS u of a beta block is (row tid / VB + 16 u, column tid % VB)
  static_assert(DEC_THREADS == 16 * VB, "beta block row slots");
  auto issue_tile = [&](int tile) {
    const int c0 = tile * VB, c = min(c0 + (tid & (VB - 1)), V - 1);
#pragma unroll
    for (int u = 0; u < BU; ++u) {
      // 32-bit element offsets (K V < 2^31): one VGPR per address, not a pair
      br[u] = m.beta[min(tid / VB + 16 * u, K - 1) * m.ldb + c];
    }
    const int v = min(c0 + col, V - 1);
    rmr = m.beta_rm[v];
    rvr = m.beta_rv[v];
  };
  if ((int)gfk_bx() < m.n_tiles) issue_tile(gfk_bx());
#pragma unroll 1
  for (int tile = gfk_bx(); tile < m.n_tiles; tile += gridDim.x) {
  const int c0 = tile * VB;
  const int v = c0 + col;
  const bool valid = v < V;
  GFK_STAMP(m, 21);
  // ---- staging: the registers of this tile -> LDS ----
  if (tile != (int)gfk_bx()) lds_barrier();      // previous tile's bt / colp reads done
  {
    const int c = tid & (VB - 1), cok = c0 + c < V;
#pragma unroll
    for (int u = 0; u < BU; ++u) {
      const int k = tid / VB + 16 * u;
      if (k < KP) bt[k * LDB_F + c] = (k < K && cok) ? br[u] : 0.f;
    }
  }
  const float rm0 = rmr, rv0 = rvr;
  if (tile == (int)gfk_bx()) vm_barrier();       // + theta_d (LDS-DMA)
  else lds_barrier();
  GFK_STAMP(m, 17);
  asm volatile("" : "+v"(tid));
  __builtin_assume(tid >= 0 && tid < DEC_THREADS);   // (unsigned index math: shifts, not
                                                      // signed-division sequences)
  if (tile + (int)gridDim.x < m.n_tiles) issue_tile(tile + gridDim.x);
  // ---- logits for this wave's row tiles x 16 columns (two independent MFMA chains) ----
  f32x4 acc[NRT];
  if constexpr (BF) {
#pragma unroll
    for (int i = 0; i < NRT; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float* ap0 = th + (rt0 * 16 + (lane & 15)) * KT;
    if (rt0 < RT) {
      // K in steps of 32 (16x16x32), a tail of 16 when KP % 32 == 16 (16x16x16)
      int k0 = 0;
      {
        const int kq = 8 * (lane >> 4);
        const float* bp = bt + kq * LDB_F + col;
        const float* ap = ap0 + kq;
        for (; k0 + 32 <= KP; k0 += 32) {
          float b[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) b[j] = bp[(k0 + j) * LDB_F];
#pragma unroll
          for (int i = 0; i < NRT; ++i)
            if (rt0 + 4 * i < RT) {
              float a[8];     // theta_d rows hold kt >= K columns: mask the K..16-padding
#pragma unroll
              for (int j = 0; j < 8; ++j) a[j] = k0 + kq + j < K ? ap[i * 64 * KT + k0 + j] : 0.f;
              acc[i] = mfma16x16x32bf(a, b, acc[i]);
            }
        }
      }
      if (k0 < KP) {
        const int kq = 4 * (lane >> 4);
        const float* bp = bt + kq * LDB_F + col;
        const float* ap = ap0 + kq;
        float b[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) b[j] = bp[(k0 + j) * LDB_F];
#pragma unroll
        for (int i = 0; i < NRT; ++i)
          if (rt0 + 4 * i < RT) {
            float a[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) a[j] = k0 + kq + j < K ? ap[i * 64 * KT + k0 + j] : 0.f;
            acc[i] = mfma16x16x16bf(a, b, acc[i]);
          }
      }
    }
  } else {
    f32x4 acc2[NRT];
#pragma unroll
    for (int i = 0; i < NRT; ++i) acc[i] = acc2[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float* bp = bt + (lane >> 4) * LDB_F + col;
    const float* ap = th + (rt0 * 16 + (lane & 15)) * KT + (lane >> 4);
    if (rt0 < RT) {
      int k0 = 0;
      for (; k0 + 4 < KP; k0 += 8) {
        const float b0 = bp[k0 * LDB_F], b1 = bp[(k0 + 4) * LDB_F];
#pragma unroll
        for (int i = 0; i < NRT; ++i)
          if (rt0 + 4 * i < RT) {
            acc[i] = mfma16x16x4(ap[i * 64 * KT + k0], b0, acc[i]);
            acc2[i] = mfma16x16x4(ap[i * 64 * KT + k0 + 4], b1, acc2[i]);
          }
      }
      if (k0 < KP) {
        const float b0 = bp[k0 * LDB_F];
#pragma unroll
        for (int i = 0; i < NRT; ++i)
          if (rt0 + 4 * i < RT) acc[i] = mfma16x16x4(ap[i * 64 * KT + k0], b0, acc[i]);
      }
    }
#pragma unroll
    for (int i = 0; i < NRT; ++i) acc[i] += acc2[i];
  }
  GFK_STAMP(m, 18);

  // ---- column batch-norm: wave partials over its rows, combined through LDS ----
  const float inv_nb = 1.f / (float)nb;
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < NRT; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int row = (rt0 + 4 * i) * 16 + (lane >> 4) * 4 + e;
      s += (row < nb && rt0 + 4 * i < RT) ? acc[i][e] : 0.f;
    }
  s = sum_groups(s);
  if (lane < 16) colp[rt0 * VB + col] = s;
  lds_barrier();
  const float mean = (colp[col] + colp[VB + col] + colp[2 * VB + col] + colp[3 * VB + col]) * inv_nb;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < NRT; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int row = (rt0 + 4 * i) * 16 + (lane >> 4) * 4 + e;
      const float d = acc[i][e] - mean;
      q += (row < nb && rt0 + 4 * i < RT) ? d * d : 0.f;
    }
  q = sum_groups(q);
  if (lane < 16) colq[rt0 * VB + col] = q;
  lds_barrier();
  const float var = (colq[col] + colq[VB + col] + colq[2 * VB + col] + colq[3 * VB + col]) * inv_nb;
  const float rstd = rsqrtf(var + m.bn_eps);
  if (rt0 == 0 && lane < 16 && valid) {
    const float mom = m.bn_momentum;
    const float unb = nb > 1 ? var * (float)nb / (float)(nb - 1) : var;
    float nm = (1.f - mom) * rm0 + mom * mean, nv = (1.f - mom) * rv0 + mom * unb;
    if (m.fed_scale_on && is_shared(m, m.beta_rm)) { nm *= m.fed_scale; nv *= m.fed_scale; }
    m.beta_rm[v + gfk_own<GB>(m)] = nm;
    m.beta_rv[v + gfk_own<GB>(m)] = nv;
    m.ws_col_rstd[v] = rstd;
  }
  GFK_STAMP(m, 19);

  // ---- normalise, store the BN'ed tile, accumulate the per-row sum of exp ----
  float* zt = m.ws_zn + (size_t)tile * BM * VB;
#pragma unroll
  for (int i = 0; i < NRT; ++i) {
    if (rt0 + 4 * i >= RT) continue;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int row = (rt0 + 4 * i) * 16 + (lane >> 4) * 4 + e;
      const float z = (acc[i][e] - mean) * rstd;
      if (row < nb) zt[row * VB + (col ^ zswz(row))] = z;
      rs_[i][e] += valid ? __expf(z) : 0.f;
    }
  }
  GFK_STAMP(m, 20);
  }
  // ---- this workgroup's per-row partials (one per wave column strip) ----
  float* part = m.ws_row_part + (size_t)(gfk_bx() * 4 + cs) * m.bmax * 2;
#pragma unroll
  for (int i = 0; i < NRT; ++i) {
    if (rt0 + 4 * i >= RT) continue;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int row = (rt0 + 4 * i) * 16 + (lane >> 4) * 4 + e;
      const float se = row16_sum(rs_[i][e]);
      if ((lane & 15) == 0 && row < nb) {
        part[2 * row] = 0.f;                   // (max, sum-exp) partial with max 0
        part[2 * row + 1] = se;
      }
    }
  }
}

// Strip forward (fp32, B <= 64; stage_flags bit 2, the engine's default where it
// applies).  The tile kernel above runs its phases serially per tile -- staging, MFMA,
// two batch-norm barriers, stores.  Here each WAVE owns a 16-column strip of a vocab
// tile for ALL batch rows and works through its strips independently:
//  * the MFMA B operand (beta, the strip's 16 columns x K) comes straight from global
//    memory into registers by buffer loads (one per-lane offset, rows past K read as 0),
//    so the LDS holds theta_d alone and no beta tile;
//  * the column batch-norm statistics are a reduction over the wave's own rows: register
//    sums + two lane-group shuffles, no LDS, no barrier;
//  * after theta_d is staged there is no barrier between the waves;
//  * the next strip's beta pairs in flight while this one runs its MFMAs (PF below).
// k pairing: MFMA steps 2t and 2t + 1 take k = 8t + 2g and 8t + 2g + 1 for lane group
// g = lane >> 4 (any bijection of k works if A and B agree), so a lane's two A operands
// are one ds_read_b64, read one pair ahead of the MFMAs.  Strips s = tile * 4 + cs are
// dealt to waves in whole tiles (the 4 strips of a tile to the 4 waves of a wave group:
// their beta rows share cache lines).  The per-row sum-exp partials of the waves are summed through LDS
// once at the end and stored as the workgroup's 4 partial slots (slot 0 holds the sum,
// 1..3 zero), so row_loss reads the same dec_grid * 4 partials as with the tile kernel.
// The first strip's beta block is issued behind theta_d's staging loads, so the two
// global rounds overlap.  Measured (profiles/r2/ab_strip_forward.txt): K=50 headline
// round 0.0589 -> 0.0583 ms, K=50 V=28k 0.101 -> 0.092, K=200 V=112k 0.349 -> 0.342.
// NP: k pairs held in registers (compile-time, the launcher's smallest instance >= K / 8).
// PF = 3 (the only variant since round 6): ROLLING prefetch at 16 waves of <= 128 VGPRs:
// right after the MFMAs that consume a k pair of this strip's beta block, the next pair is
// loaded into those registers, so each pair has many MFMAs of time to arrive, with no second
// register block.  The pairs go through a RING of strip_ring(NP) <= 13
// pairs instead of the whole strip's NP: pair t's registers receive pair t + R -- of this
// strip while t + R < NP, else of the next one -- so a load still has R pairs of MFMAs
// (x 4 waves per SIMD) to arrive, and K = 200 (25 pairs) fits 128 VGPRs: 16 waves per CU
// instead of 12, and 7004 strips over 4096 waves (at most 2 each; 76 -> 85 % of the last
// round's slots busy) instead of 3072 (at most 3).  (Round 6 removed the whole-strip rolling
// variant PF = 2 and the non-prefetching PF = 0, both measured slower: profiles/r3, r4; and
// the 8-wave variant prefetching the whole next block, PF = 1 (190 VGPRs, 2 waves per SIMD),
// the batched plan's large-V choice until then: profiles/r6/ab_strip_pf_vs_ring.txt.)
__host__ __device__ constexpr int strip_threads(int pf, int np) { return 1024; }
// The ring must divide NP: the next strip's pair p is written into the slot of pair
// p + NP - R of this one, and read back from slot p % R.  (A 13-pair ring with NP = 25
// -- K = 200 until round 4 -- shifted every later strip's beta pairs by one slot: wrong
// logits wherever a wave had a second strip, i.e. more than 4096 strips, V > 65k.)
__host__ __device__ constexpr int strip_ring(int pf, int np) {
  if (pf != 3 || np <= 13) return np;
  int d = 13;
  while (np % d) --d;
  return d;
}
// (GFK_STAMPS builds: per-wave timeline of workgroups 0 and grid-1, tools/stamps.py)
#ifdef GFK_STAMPS
#define STRIP_STAMP(j, rt)                                                                \
  do {                                                                                    \
    __builtin_amdgcn_sched_barrier(0);                                                    \
    if ((gfk_bx() == 0 || gfk_bx() == gridDim.x - 1) && lane == 0 && m.dbg)           \
      m.dbg[64 + (gfk_bx() ? 16 * 16 : 0) + wave * 16 + (j)] =                          \
          (rt) ? __builtin_amdgcn_s_memrealtime() : __builtin_amdgcn_s_memtime();         \
    __builtin_amdgcn_sched_barrier(0);                                                    \
  } while (0)
#else
#define STRIP_STAMP(j, rt) do { } while (0)
#endif
// BF (mm_bf16, PF = 3 only): the logits on v_mfma_f32_16x16x32_bf16 -- pairs t = 4 s + u hold
// k = 32 s + 8 g + 2 u (+ 1) for lane group g, so the 4 pairs of step s are the 8 consecutive
// k of the lane's B operand (B[8 g + j][col]); A = 8 consecutive k of theta_d's row from LDS
// (two ds_read_b128); both rounded to bf16 in registers, fp32 accumulation.  16x fewer MFMA
// cycles than the fp32 path, which is what bounds it at K = 200 (not the beta stream).
//
// FP (stage_flags GFK_FWD_POSTFOLD; ring variant, K <= 64, no label head): the batch-coupled
// posterior of post_fwd runs here, in the theta_d staging phase, and post_fwd is not launched
// (one kernel boundary and one dependent round trip less per step).  Every workgroup
// loads the raw [B, 2K] heads (mu | log sigma^2, 2 B K floats from L2), its rows' noise and
// dropout masks, computes the column batch-norm statistics, and for every row the
// normalised heads, the reparameterised sample, softmax(theta) and theta_d = theta * mask
// straight into its LDS theta_d block -- redundant across workgroups, but a few KB of
// reads and ~2 B K exps instead of a launch.  Row r's outputs for the backward (mu, log
// sigma^2, theta, theta_d, KL) are stored by workgroup r % grid only; workgroup 0 advances
// the running statistics, the counters and the optimizer step, as post_fwd's row 0 did.
// Same arithmetic as gfk_post_fwd_k (csrc/posterior.hip; reference inference_network.py:
// 82-83 + decoder_network.py:102-118 + avitm.py:207-220).
template <int BM, int NP, int PF, bool GB = false, bool BF = false, bool FP = false>
__global__ void __launch_bounds__(strip_threads(PF, NP)) prodlda_fwd_strip_kernel(GfkArgT<GB> ga) {
  static_assert(PF == 3, "strip variant: the ring (3)");
  static_assert(!BF || (PF == 3 && NP % 4 == 0), "bf16 strips: ring variant, whole 32-k steps");
  static_assert(!FP || (PF == 3 && NP == 8), "fused posterior: ring variant, K <= 64");
  const GfkModel& m = gfk_model(ga);
  constexpr int STRIP_THREADS = strip_threads(PF, NP);
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int K = m.K, V = m.V, KT = m.kt;
  const int LDB = uniform(m.ldb);              // beta's row stride (>= V)
  int tid = threadIdx.x;
  const int lane = tid & 63, wave = uniform(tid >> 6);
  constexpr int RT = BM / 16;
  constexpr int NW = STRIP_THREADS / 64;
  STRIP_STAMP(0, false);
  STRIP_STAMP(1, true);
  // theta_d re-staged with its own row stride KS = 8 NP + 4 (4 x odd: ds_read_b64 banks
  // lanes {0-31} / {32-63} over 64 banks, and rows r * KS of 16 lanes + the two lane
  // groups' k offsets 2g then cover all 64 -- measured 45 % conflicted cycles with the
  // 2 x odd stride a 32-bank layout would want) and ZERO beyond K and in
  // rows >= nb: the MFMA loop then needs no k masks (pairs past K multiply zero A and
  // zero B) and the rows >= nb contribute exact zeros to the logits
  constexpr int KS = 8 * NP + 4;
  float* th = smem;                            // [BM][KS]
  float* red = th + BM * KS;                   // [NW][BM] per-wave row partials
  float rs_[RT][4];
#pragma unroll
  for (int i = 0; i < RT; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) rs_[i][e] = 0.f;

  const int nb = *m.ws_nb;
  if (gfk_bx() == 0 && tid == 0) *m.nbt_beta += 1;
  const int g2 = 2 * (lane >> 4);
  const int gb = BF ? 8 * (lane >> 4) : g2;    // the lane group's first beta row
  // first beta row of pair t (relative to gb)
  auto prow = [](int t) constexpr { return BF ? 32 * (t >> 2) + 2 * (t & 3) : 8 * t; };
  const float inv_nb = 1.f / (float)nb;
  const int nstrips = m.n_tiles * 4;
  const int stride = gridDim.x * NW;
  const int arow = (lane & 15) * KS + (BF ? gb : g2);
  // beta [K, V] as a buffer resource of K V floats (K V < 2^29 checked by the launcher)
  const __amdgpu_buffer_rsrc_t bres =
      __builtin_amdgcn_make_buffer_rsrc((void*)m.beta, 0, K * LDB * 4, 0x00020000);
  // A strip's beta block into registers: buffer loads with ONE per-lane offset (row g2,
  // column) stepped by 8 rows per pair; rows k >= K lie past the resource's extent and
  // read as 0 (no clamps, no per-load address VGPRs).  Unconditional: a guarded load
  // becomes a branch + vmcnt(0) per pair in the ISA.  The row step is made opaque per
  // call so the offsets are recomputed here, not hoisted out of the loop and spilled.
  auto issue = [&](int st, auto& bb, float& rm, float& rv) {
    constexpr int NL = sizeof(bb) / sizeof(float) / 2;    // pairs: NR (the ring) or NP
    const int vc = min((st >> 2) * VB + 16 * (st & 3) + (lane & 15), V - 1);
    int v4 = LDB * 4;
    asm volatile("" : "+s"(v4));
    int voff = gb * v4 + vc * 4;
#pragma unroll
    for (int t = 0; t < NL; ++t) {
      bb[2 * t] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(bres, voff, 0, 0));
      bb[2 * t + 1] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(bres, voff, v4, 0));
      if (t + 1 < NL) voff += (prow(t + 1) - prow(t)) * v4;
    }
    rm = m.beta_rm[vc];
    rv = m.beta_rv[vc];
  };
  // software pipeline over the wave's strips: the NEXT strip's first beta pairs are in
  // flight while this one runs its last MFMAs / batch norm / stores
  constexpr int NR = strip_ring(PF, NP);       // pairs held in registers
  static_assert(NP % NR == 0, "the ring's slots must repeat whole strips");
  float b[2 * NR], rm0 = 0.f, rv0 = 0.f, rmn = 0.f, rvn = 0.f;
  // wave group gq = wave >> 2 takes whole tiles gq * grid + g, + NW / 4 * grid, ...: the
  // 4 strips of a tile stay on one CU (their beta rows share cache lines), and the
  // tiles of the last, partial round are spread over every CU's wave group 0 instead
  // of all 8 waves of the first CUs, so no SIMD gets more than ceil(strips / SIMDs) + 1
  int s = 4 * ((wave >> 2) * (int)gridDim.x + (int)gfk_bx()) + (wave & 3);
  if constexpr (FP) {
    // ---- fused posterior: one round of loads (heads, the rows' noise / masks, priors,
    // workgroup 0's running statistics and counters), the first beta block behind them ----
    static_assert(BM % NW == 0, "whole rows per wave");
    constexpr int RPW = BM / NW;                 // rows per wave
    constexpr int HU = (2 * BM * 64 + STRIP_THREADS - 1) / STRIP_THREADS;
    constexpr int CPASS = 2;                     // 2K <= 128 columns, 64 per pass
    float* hm = red + NW * BM;                   // [2][BM][K]: mu_raw | ls_raw
    float* cm = hm + 2 * BM * 64;                // [128] column means
    float* cr = cm + 128;                        // [128] column rstd
    const int BK = BM * K;
    float hv[HU];
#pragma unroll
    for (int u = 0; u < HU; ++u) {
      const int e = min(tid + u * STRIP_THREADS, 2 * BK - 1);
      const float* src = e < BK ? m.ws_mu_raw + e : m.ws_ls_raw + (e - BK);
      hv[u] = *src;
    }
    const int kc = min(lane, K - 1);
    float ep[RPW], mk[RPW];
#pragma unroll
    for (int i = 0; i < RPW; ++i) {
      const int r = wave + NW * i;
      ep[i] = m.ws_eps[r * K + kc];
      mk[i] = m.ws_mask_t[r * K + kc];
    }
    const float pmk = m.prior_mean[kc], pvk = m.prior_var[kc];
    // (unconditional: every workgroup loads them, workgroup 0 uses them -- a load behind a
    // branch would make the waitcnt pass drain the beta block below at its first use)
    float rmp[CPASS], rvp[CPASS];
#pragma unroll
    for (int p = 0; p < CPASS; ++p) {
      const int c2 = min(p * 64 + (tid >> 4), 2 * K - 1);
      rmp[p] = c2 < K ? m.mu_rm[c2] : m.s_rm[c2 - K];
      rvp[p] = c2 < K ? m.mu_rv[c2] : m.s_rv[c2 - K];
    }
    const double pw0 = m.adam_pow[0], pw1 = m.adam_pow[1];
    const int64_t nbt0 = *m.nbt_mu, nbt1 = *m.nbt_s;
    const int32_t at0 = *m.adam_t;
    if (PF != 0) issue(min(s, nstrips - 1), b, rm0, rv0);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < HU; ++u)
      if (tid + u * STRIP_THREADS < 2 * BK) hm[tid + u * STRIP_THREADS] = hv[u];
    lds_barrier();
    // ---- column batch-norm statistics of the 2K heads over the nb rows: 16 lanes per
    // column (rows g, g + 16, ..), 64 columns per pass ----
    const bool w0 = gfk_bx() == 0;
#pragma unroll
    for (int p = 0; p < CPASS; ++p) {
      if (p * 64 >= 2 * K) break;
      const int c2 = p * 64 + (tid >> 4), g = tid & 15;
      const bool valid = c2 < 2 * K;
      const int cc = min(c2, 2 * K - 1);
      const float* x = hm + (cc < K ? cc : BK + (cc - K));
      constexpr int RPT = BM / 16;
      float xv[RPT], sm = 0.f;
#pragma unroll
      for (int i = 0; i < RPT; ++i) {
        const int r = g + 16 * i;
        xv[i] = r < nb ? x[r * K] : 0.f;
        sm += xv[i];
      }
      const float mean = row16_sum(sm) * inv_nb;
      float q = 0.f;
#pragma unroll
      for (int i = 0; i < RPT; ++i) {
        const float d = g + 16 * i < nb ? xv[i] - mean : 0.f;
        q += d * d;
      }
      const float var = row16_sum(q) * inv_nb;
      const float rstd = rsqrtf(var + m.bn_eps);
      if (valid && g == 0) {
        cm[c2] = mean;
        cr[c2] = rstd;
        if (w0) {
          const int k = c2 < K ? c2 : c2 - K;
          float* rmq = c2 < K ? m.mu_rm + k : m.s_rm + k;
          float* rvq = c2 < K ? m.mu_rv + k : m.s_rv + k;
          const float mom = m.bn_momentum;
          const float unb = nb > 1 ? var * (float)nb / (float)(nb - 1) : var;
          float nm = (1.f - mom) * rmp[p] + mom * mean, nv = (1.f - mom) * rvp[p] + mom * unb;
          if (m.fed_scale_on && is_shared(m, rmq)) { nm *= m.fed_scale; nv *= m.fed_scale; }
          rmq[gfk_own<GB>(m)] = nm;
          rvq[gfk_own<GB>(m)] = nv;
          m.ws_bn_rstd[c2] = rstd;
        }
      }
    }
    if (w0 && tid == 0) {
      *m.nbt_mu = nbt0 + 1;
      *m.nbt_s = nbt1 + 1;
      *m.adam_t = at0 + 1;                       // the optimizer step of this minibatch
      double p1, p2;
      float c0, c1;
      adam_advance(m, pw0, pw1, p1, p2, c0, c1);
      m.adam_pow[0] = p1;
      m.adam_pow[1] = p2;
      m.adam_coef[0] = c0;
      m.adam_coef[1] = c1;
    }
    lds_barrier();
    // ---- per row (wave w: rows w, w + NW, ..; lane = topic): normalise, reparameterise,
    // softmax, dropout -> theta_d in LDS (zero past K and in rows >= nb); the row's
    // writer workgroup stores what row_bwd / post_bwd / the backward read ----
    const int KTs = KT;
#pragma unroll
    for (int i = 0; i < RPW; ++i) {
      const int r = wave + NW * i;
      const bool live = r < nb;
      float mu = 0.f, ls = 0.f, z = -INFINITY, klt = 0.f, lpv = 0.f;
      if (lane < K) {
        mu = (hm[r * K + lane] - cm[lane]) * cr[lane];
        ls = (hm[BK + r * K + lane] - cm[K + lane]) * cr[K + lane];
        const float sd = expf(0.5f * ls);
        z = mu + ep[i] * sd;
        const float dm = pmk - mu;
        klt = sd * sd / pvk + dm * dm / pvk - ls;
        lpv = logf(pvk);
      }
      const float zmax = wave_max(z);
      const float ez = lane < K ? expf(z - zmax) : 0.f;
      const float tht = ez * (1.f / wave_sum(ez));
      const float thd = tht * mk[i];
      th[r * KS + lane] = (live && lane < K) ? thd : 0.f;
      if (lane < KS - 64) th[r * KS + 64 + lane] = 0.f;
      if (live && r % (int)gridDim.x == (int)gfk_bx()) {
        if (lane < K) {
          m.ws_mu[r * K + lane] = mu;
          m.ws_ls[r * K + lane] = ls;
          m.ws_theta[r * K + lane] = tht;
          m.ws_thetad[r * KTs + lane] = thd;
        }
        const float kl = wave_sum(klt), lp = wave_sum(lpv);
        if (lane == 0) m.ws_kl[r] = 0.5f * (kl - (float)K + lp);
      }
    }
  } else {
    constexpr int SU = (BM * KS + STRIP_THREADS - 1) / STRIP_THREADS;
    float tv[SU];
#pragma unroll
    for (int u = 0; u < SU; ++u) {
      // (clamped, unconditional loads: a guarded load compiles to a branch + vmcnt(0))
      const int idx = tid + u * STRIP_THREADS, row = idx / KS, k = idx % KS;
      tv[u] = m.ws_thetad[min(row, BM - 1) * KT + min(k, K - 1)];
    }
    // the first strip's beta block is issued BEHIND theta_d's loads: waiting for those
    // (vmcnt counts in order) leaves it in flight across the staging barrier, so the
    // two global rounds overlap instead of following each other
    // (unconditional, clamped: behind a branch the waitcnt pass would assume the loads
    // absent at the join and wait for everything)
    if (PF != 0) issue(min(s, nstrips - 1), b, rm0, rv0);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < SU; ++u) {
      // an integer mask, not a select: a select lets the compiler sink the load into a
      // branch (+ vmcnt(0) each), and 0 * x would keep a NaN of the unused rows
      const int idx = tid + u * STRIP_THREADS, row = idx / KS, k = idx % KS;
      const unsigned keepm = (row < nb && k < K) ? ~0u : 0u;
      tv[u] = __uint_as_float(__float_as_uint(tv[u]) & keepm);
    }
#pragma unroll
    for (int u = 0; u < SU; ++u)
      if (tid + u * STRIP_THREADS < BM * KS) th[tid + u * STRIP_THREADS] = tv[u];
  }
  lds_barrier();
  STRIP_STAMP(2, false);
  asm volatile("" : "+v"(tid));
  __builtin_assume(tid >= 0 && tid < STRIP_THREADS);
#ifdef GFK_STAMPS
  int it_ = 0;
#endif
  // PF = 3: this strip's per-lane offset of pair 0 (its pairs R.. are loaded in the loop)
  int voffc = 0;
  if (PF == 3) {
    const int s0 = min(s, nstrips - 1);
    const int vc0 = min((s0 >> 2) * VB + 16 * (s0 & 3) + (lane & 15), V - 1);
    voffc = gb * (LDB * 4) + vc0 * 4;
  }
#pragma unroll 1
  for (; s < nstrips; s += stride) {
    // PF = 3: the next strip's per-lane buffer offset (its pairs are loaded in the MFMA loop)
    int voffn = 0, v4n = LDB * 4;
    {
      const int sn = min(s + stride, nstrips - 1);
      const int vcn = min((sn >> 2) * VB + 16 * (sn & 3) + (lane & 15), V - 1);
      asm volatile("" : "+s"(v4n));
      voffn = gb * v4n + vcn * 4;
      rmn = m.beta_rm[vcn];
      rvn = m.beta_rv[vcn];
    }
    const int tile = s >> 2, cs = s & 3;
    const int col = 16 * cs + (lane & 15);
    const int v = tile * VB + col;
    const bool valid = v < V;
    int aoff = arow;                  // (an integer: an opaque pointer would turn the
    asm volatile("" : "+v"(aoff));    //  LDS reads into FLAT loads)
    const float* ap = th + aoff;
    // ---- logits [BM, 16] on the matrix cores: RT independent accumulation chains ----
    f32x4 acc[RT];
#pragma unroll
    for (int i = 0; i < RT; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    // (NP is the launcher's smallest instance >= the pairs of K; the pairs past K are
    // zero in both operands)
    // A reads one pair ahead of the MFMAs (double-buffered registers); the fences keep
    // the scheduler from hoisting every pair's reads above the first MFMA (spills)
    if constexpr (BF) {
#pragma unroll
      for (int st = 0; st < NP / 4; ++st) {
        __builtin_amdgcn_sched_barrier(0);
        float b8[8];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          b8[2 * u] = b[2 * ((4 * st + u) % NR)];
          b8[2 * u + 1] = b[2 * ((4 * st + u) % NR) + 1];
        }
#pragma unroll
        for (int i = 0; i < RT; ++i) {
          const f32x4 lo = *reinterpret_cast<const f32x4*>(ap + i * 16 * KS + 32 * st);
          const f32x4 hi = *reinterpret_cast<const f32x4*>(ap + i * 16 * KS + 32 * st + 4);
          const float a8[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
          acc[i] = mfma16x16x32bf(a8, b8, acc[i]);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {       // pair t + NR (this strip's, else the next one's)
          const int t = 4 * st + u, pn = t + NR;
          const int vo = pn < NP ? voffc + prow(pn) * v4n : voffn + prow(pn - NP) * v4n;
          b[2 * (t % NR)] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(bres, vo, 0, 0));
          b[2 * (t % NR) + 1] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(bres, vo, v4n, 0));
        }
      }
    } else {
    float2 a[2][RT];
#pragma unroll
    for (int i = 0; i < RT; ++i) a[0][i] = *reinterpret_cast<const float2*>(ap + i * 16 * KS);
#pragma unroll
    for (int t = 0; t < NP; ++t) {
      __builtin_amdgcn_sched_barrier(0);
      if (t + 1 < NP) {
#pragma unroll
        for (int i = 0; i < RT; ++i)
          a[(t + 1) & 1][i] = *reinterpret_cast<const float2*>(ap + i * 16 * KS + 8 * (t + 1));
      }
#pragma unroll
      for (int i = 0; i < RT; ++i) acc[i] = mfma16x16x4(a[t & 1][i].x, b[2 * (t % NR)], acc[i]);
#pragma unroll
      for (int i = 0; i < RT; ++i) acc[i] = mfma16x16x4(a[t & 1][i].y, b[2 * (t % NR) + 1], acc[i]);
      if (PF == 3) {                  // pair t + NR (this strip's, else the next one's)
        const int pn = t + NR;
        const int vo = pn < NP ? voffc + pn * 8 * v4n : voffn + (pn - NP) * 8 * v4n;
        b[2 * (t % NR)] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(bres, vo, 0, 0));
        b[2 * (t % NR) + 1] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(bres, vo, v4n, 0));
      }
    }
    }
    if (PF == 3) voffc = voffn;
#ifdef GFK_STAMPS
    if (it_ < 2) STRIP_STAMP(3 + 2 * it_, false);
#endif
    // ---- column batch-norm over the wave's own rows (rows >= nb excluded) ----
    // (rows >= nb are exact zeros, so the sum needs no mask; lim is made opaque per strip
    // so the 4 RT row compares are not hoisted out of the loop as live SGPR masks)
    float sm = 0.f;
#pragma unroll
    for (int i = 0; i < RT; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) sm += acc[i][e];
    const float mean = sum_groups(sm) * inv_nb;
#ifdef GFK_STAMPS
    if (it_ == 0) STRIP_STAMP(9, false);
#endif
    int lim = nb - (lane >> 4) * 4;
    asm volatile("" : "+v"(lim));
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < RT; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float d = acc[i][e] - mean;
        q += i * 16 + e < lim ? d * d : 0.f;
      }
    const float var = sum_groups(q) * inv_nb;
    const float rstd = rsqrtf(var + m.bn_eps);
#ifdef GFK_STAMPS
    if (it_ == 0) STRIP_STAMP(10, false);
#endif
    if (lane < 16 && valid) {
      const float mom = m.bn_momentum;
      const float unb = nb > 1 ? var * (float)nb / (float)(nb - 1) : var;
      float nm = (1.f - mom) * rm0 + mom * mean, nv = (1.f - mom) * rv0 + mom * unb;
      if (m.fed_scale_on && is_shared(m, m.beta_rm)) { nm *= m.fed_scale; nv *= m.fed_scale; }
      m.beta_rm[v + gfk_own<GB>(m)] = nm;
      m.beta_rv[v + gfk_own<GB>(m)] = nv;
      m.ws_col_rstd[v] = rstd;
    }
#ifdef GFK_STAMPS
    if (it_ == 0) STRIP_STAMP(11, false);
#endif
    // ---- normalise, store the BN'ed strip, accumulate the per-row sum of exp ----
    float* zt = m.ws_zn + (size_t)tile * BM * VB;
#pragma unroll
    for (int i = 0; i < RT; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int row = i * 16 + (lane >> 4) * 4 + e;
        const float z = (acc[i][e] - mean) * rstd;
        if (i * 16 + e < lim) zt[row * VB + (col ^ zswz(row))] = z;
        rs_[i][e] += valid ? __expf(z) : 0.f;
      }
    rm0 = rmn;
    rv0 = rvn;
#ifdef GFK_STAMPS
    if (it_ < 2) STRIP_STAMP(4 + 2 * it_, false);
    ++it_;
#endif
  }
  STRIP_STAMP(7, false);
  STRIP_STAMP(8, true);
  // ---- the 16 waves' per-row partials -> the workgroup's partial slots ----
#pragma unroll
  for (int i = 0; i < RT; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float se = row16_sum(rs_[i][e]);
      if ((lane & 15) == 0) red[wave * BM + i * 16 + (lane >> 4) * 4 + e] = se;
    }
  lds_barrier();
  if (tid < 4 * BM) {
    const int slot = tid / BM, row = tid % BM;
    float se = 0.f;
    if (slot == 0)
#pragma unroll
      for (int w = 0; w < NW; ++w) se += red[w * BM + row];
    if (row < nb) {
      float* part = m.ws_row_part + ((size_t)(gfk_bx() * 4 + slot) * m.bmax + row) * 2;
      part[0] = 0.f;
      part[1] = se;
    }
  }
}

// One wave per batch row: log-sum-exp from the per-wave partials, the sparse
// reconstruction loss and S_b over the row's non-zeros (read from the row slots
// prepared with the batch, so the logit gathers are the second round trip).
template <bool GB = false>
__global__ void __launch_bounds__(64) gfk_prodlda_row_loss(GfkArgT<GB> ga) {
  const GfkModel& m = gfk_model(ga);
  int n_tiles = m.n_tiles, bmax = m.bmax;
  const int32_t *nbp = m.ws_nb, *erange = m.ws_erange;
  const float *row_part = m.ws_row_part, *zn = m.ws_zn;
  keep(n_tiles, bmax, nbp, erange, row_part, zn);
  const int b = gfk_bx(), lane = threadIdx.x;
  // ---- round 1: batch size, the row's extent, LSE partials, its non-zeros (slots) ----
  const int nb = *nbp;
  const int np = m.dec_grid * 4;                 // per-workgroup partials of prodlda_fwd
  const int e0 = erange[2 * b], e1 = erange[2 * b + 1];
  constexpr int PU = 8, SU = 4;
  float pm[PU], ps[PU];
#pragma unroll
  for (int u = 0; u < PU; ++u) {
    const int g = min(lane + 64 * u, np - 1);
    const float2 p = *reinterpret_cast<const float2*>(row_part + ((size_t)g * bmax + b) * 2);
    pm[u] = p.x;
    ps[u] = p.y;
  }
  const int cap = m.slot_cap;
  const int32_t* sidx = m.ws_sidx + (size_t)b * cap;
  const float* sval = m.ws_sval + (size_t)b * cap;
  int ci[SU];
  float xv[SU];
#pragma unroll
  for (int u = 0; u < SU; ++u) {
    const int j = min(lane + 64 * u, cap - 1);
    ci[u] = sidx[j];
    xv[u] = sval[j];
  }
  if (b >= nb) return;
  const int n = e1 - e0;
  // ---- round 2: the BN'ed logits at the non-zeros ----
  const size_t tstride = (size_t)bmax * VB;
  const float* zr = zn + (size_t)b * VB;
  float zv[SU];
#pragma unroll
  for (int u = 0; u < SU; ++u) {
    const int c = ci[u];
    zv[u] = lane + 64 * u < n ? zr[(size_t)(c / VB) * tstride + ((c % VB) ^ zswz(b))] : 0.f;
  }
  float mx = -INFINITY, se = 0.f;
#pragma unroll
  for (int u = 0; u < PU; ++u)
    if (lane + 64 * u < np) lse_merge(mx, se, pm[u], ps[u]);
  for (int g = lane + 64 * PU; g < np; g += 64) {
    const float2 p = *reinterpret_cast<const float2*>(row_part + ((size_t)g * bmax + b) * 2);
    lse_merge(mx, se, p.x, p.y);
  }
  wave_lse(mx, se);
  const float lse = mx + logf(se);
  float rl = 0.f, S = 0.f;
#pragma unroll
  for (int u = 0; u < SU; ++u) {
    if (lane + 64 * u >= n) continue;
    const float p = expf(zv[u] - lse);
    rl += xv[u] * logf(p + RL_EPS);
    S += xv[u] * p / (p + RL_EPS);
  }
  for (int j = lane + 64 * SU; j < n; j += 64) {    // rows of more than 256 non-zeros
    const int c = sidx[j];
    const float x = sval[j];
    const float p = expf(zr[(size_t)(c / VB) * tstride + ((c % VB) ^ zswz(b))] - lse);
    rl += x * logf(p + RL_EPS);
    S += x * p / (p + RL_EPS);
  }
  rl = wave_sum(rl);
  S = wave_sum(S);
  if (lane == 0) {
    m.ws_lse[b] = lse;
    m.ws_rl[b] = -rl;
    m.ws_s[b] = S;
  }
}

// ---------------------------------------------------------------------------
// Large batches (stage_flags GFK_LB, bmax 256 / 512; csrc/gfk_common.h).  The decoder's three
// products are library GEMMs the engine issues on the step's stream (at B >= 256 they are
// big enough for hipBLASLt to run them near the matrix cores' peak): logits = theta_d beta
// into ws_dt as a plain [bmax][ldb] matrix, then dbeta = theta_d^T dlogit (beta's gradient
// slot) and d theta_d = dlogit beta^T (slab 0) from the logit gradient these kernels leave
// in ws_dt.  What is batch-coupled around them runs here:
//   prodlda_lb_colbn  : column batch-norm of the logits over the batch (+ running statistics,
//                       rstd), the BN'ed tile into ws_zn (row_loss's layout), per-row
//                       sum-exp partials (the same ws_row_part layout as the forward kernels);
//   prodlda_lb_dlogit : the logit gradient -- dense p S_b, the sparse -x p / (p + 1e-10) at
//                       the row's non-zeros of the tile, the column BN backward -- over the
//                       logits in ws_dt (rows >= nb and padding columns zero: the GEMMs read
//                       the whole matrix).
// Layout: thread (wave w, lane c) owns column c of a 64-column tile and rows w + 16 i, so
// every global access of a wave is one 256-B row segment, a row's sparse entries are handled
// by the one wave that owns the row (a wave-uniform loop: the owning lane adds the term --
// no LDS tile, no barrier), and the column sums reduce over the 16 waves through LDS.
// grid: dec_grid workgroups of 1024 threads, persistent over the tiles.
// ---------------------------------------------------------------------------
constexpr int LB_THREADS = 1024;

template <int BM, bool GB = false>
__global__ void __launch_bounds__(LB_THREADS) prodlda_lb_colbn_kernel(GfkArgT<GB> ga) {
  const GfkModel& m = gfk_model(ga);
  constexpr int NR = BM / 16;
  __shared__ float red[2][16][VB];
  const int tid = threadIdx.x, lane = tid & 63, w = uniform(tid >> 6);
  const int V = m.V, ldb = m.ldb, nb = *m.ws_nb;
  const float inv_nb = 1.f / (float)nb;
  // the logits / zn through buffer descriptors: a row's offset is wave-uniform (the scalar
  // offset), the column's the one vector offset -- no 64-bit address per row in registers
  const __amdgpu_buffer_rsrc_t rl = __builtin_amdgcn_make_buffer_rsrc(
      (void*)m.ws_dt, 0, (int)((size_t)m.bmax * ldb * 4), 0x00020000);
  if (gfk_bx() == 0 && tid == 0) *m.nbt_beta += 1;
  float rs[NR];                       // this lane's sum of exp(z) per row over its tiles
#pragma unroll
  for (int i = 0; i < NR; ++i) rs[i] = 0.f;
#pragma unroll 1
  for (int tile = gfk_bx(); tile < m.n_tiles; tile += gridDim.x) {
    const int v = tile * VB + lane, vc = min(v, V - 1);
    const bool valid = v < V;
    float rm0 = 0.f, rv0 = 0.f;
    if (w == 0) { rm0 = m.beta_rm[vc]; rv0 = m.beta_rv[vc]; }
    float x[NR], sm = 0.f;
#pragma unroll
    for (int i = 0; i < NR; ++i)
      x[i] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rl, vc * 4, min(w + 16 * i, nb - 1) * ldb * 4, 0));
#pragma unroll
    for (int i = 0; i < NR; ++i) sm += w + 16 * i < nb ? x[i] : 0.f;
    red[0][w][lane] = sm;
    __syncthreads();
    float mean = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) mean += red[0][j][lane];
    mean *= inv_nb;
    float q = 0.f;                    // two-pass variance, as torch's batch norm
#pragma unroll
    for (int i = 0; i < NR; ++i) {
      const float d = x[i] - mean;
      q += w + 16 * i < nb ? d * d : 0.f;
    }
    red[1][w][lane] = q;
    __syncthreads();
    float var = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) var += red[1][j][lane];
    var *= inv_nb;
    const float rstd = rsqrtf(var + m.bn_eps);
    if (w == 0 && valid) {
      const float mom = m.bn_momentum;
      const float unb = nb > 1 ? var * (float)nb / (float)(nb - 1) : var;
      float nm = (1.f - mom) * rm0 + mom * mean, nv = (1.f - mom) * rv0 + mom * unb;
      if (m.fed_scale_on && is_shared(m, m.beta_rm)) { nm *= m.fed_scale; nv *= m.fed_scale; }
      m.beta_rm[v] = nm;
      m.beta_rv[v] = nv;
      m.ws_col_rstd[v] = rstd;
    }
    const __amdgpu_buffer_rsrc_t rz = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(m.ws_zn + (size_t)tile * BM * VB), 0, BM * VB * 4, 0x00020000);
    const int zc = (lane ^ zswz(w)) * 4;     // (zswz(w + 16 i) == zswz(w))
#pragma unroll
    for (int i = 0; i < NR; ++i) {
      const int r = w + 16 * i;
      const float z = (x[i] - mean) * rstd;
      if (r < nb) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(z), rz, zc, r * VB * 4, 0);
      rs[i] += (valid && r < nb) ? __expf(z) : 0.f;
    }
    // (red[0] is rewritten next tile only after every wave passed the second barrier, which
    // follows its reads; red[1]'s reads precede the next tile's first barrier)
  }
  float* part = m.ws_row_part + (size_t)gfk_bx() * 4 * m.bmax * 2;
#pragma unroll
  for (int i = 0; i < NR; ++i) {
    const int r = w + 16 * i;
    const float se = row16_sum(rs[i]);
    if ((lane & 15) == 0 && r < nb) {
      float* p = part + ((size_t)(lane >> 4) * m.bmax + r) * 2;
      p[0] = 0.f;                     // (max, sum-exp) with max 0: |z| <= sqrt(nb - 1)
      p[1] = se;
    }
  }
}

template <int BM, bool GB = false>
__global__ void __launch_bounds__(LB_THREADS) prodlda_lb_dlogit_kernel(GfkArgT<GB> ga) {
  const GfkModel& m = gfk_model(ga);
  constexpr int NR = BM / 16, RB = NR < 8 ? NR : 8;   // rows per thread; rows per load block
  __shared__ float red[2][16][VB];
  __shared__ float sx[16][VB];               // per wave: the current row's sparse x by column
  const int tid = threadIdx.x, lane = tid & 63, w = uniform(tid >> 6);
  const int V = m.V, ldb = m.ldb, nb = *m.ws_nb, ntp = m.n_tiles + 1;
  const float inv_nb = 1.f / (float)nb;
  const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc(
      (void*)m.ws_dt, 0, (int)((size_t)m.bmax * ldb * 4), 0x00020000);
  const int zc = (lane ^ zswz(w)) * 4;       // (zswz(w + 16 i) == zswz(w))
  sx[w][lane] = 0.f;
#pragma unroll 1
  for (int tile = gfk_bx(); tile < m.n_tiles; tile += gridDim.x) {
    const int c0 = tile * VB, v = c0 + lane;
    const bool valid = v < V;
    const __amdgpu_buffer_rsrc_t rz = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(m.ws_zn + (size_t)tile * BM * VB), 0, BM * VB * 4, 0x00020000);
    const float rsd = m.ws_col_rstd[min(v, V - 1)];
    // the tile extents of this wave's rows in one round: lane i holds row w + 16 i's
    int ex0 = 0, ex1 = 0;
    if (lane < NR && w + 16 * lane < nb) {
      const int32_t* ts = m.ws_tstart + (size_t)(w + 16 * lane) * ntp + tile;
      ex0 = ts[0];
      ex1 = ts[1];
    }
    float z[NR], d[NR], s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i0 = 0; i0 < NR; i0 += RB) {
      // the block's non-zeros (lane j: the row's j-th entry in this tile), z, lse, S: one round
      int ci[RB];
      float xi[RB];
#pragma unroll
      for (int i = 0; i < RB; ++i) {
        const int e0 = __builtin_amdgcn_readlane(ex0, i0 + i), n = __builtin_amdgcn_readlane(ex1, i0 + i) - e0;
        ci[i] = -1;
        xi[i] = 0.f;
        if (lane < n) {
          ci[i] = m.indices[e0 + lane] - c0;
          xi[i] = m.values[e0 + lane];
        }
        z[i0 + i] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rz, zc, (w + 16 * (i0 + i)) * VB * 4, 0));
      }
#pragma unroll
      for (int i = 0; i < RB; ++i) {
        const int r = w + 16 * (i0 + i);
        d[i0 + i] = 0.f;
        if (r < nb) {                        // (wave-uniform)
          const float p = __expf(z[i0 + i] - m.ws_lse[r]);
          // the row's sparse x to the lanes that own their columns (LDS, in wave order)
          if (ci[i] >= 0) sx[w][ci[i]] = xi[i];
          const float xs = sx[w][lane];
          sx[w][lane] = 0.f;
          const float dd = p * m.ws_s[r] - xs * p / (p + RL_EPS);
          d[i0 + i] = valid ? dd : 0.f;
          s1 += d[i0 + i];
          s2 += d[i0 + i] * z[i0 + i];
        } else {
          z[i0 + i] = 0.f;
        }
      }
    }
    red[0][w][lane] = s1;
    red[1][w][lane] = s2;
    __syncthreads();
    float a1 = 0.f, a2 = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      a1 += red[0][j][lane];
      a2 += red[1][j][lane];
    }
    a1 *= inv_nb;
    a2 *= inv_nb;
    const float rr = valid ? rsd : 0.f;
    const int vo = v < ldb ? v * 4 : 0x7FFF0000;   // (columns past ldb: dropped stores)
#pragma unroll
    for (int i = 0; i < NR; ++i) {
      const int r = w + 16 * i;
      const float o = r < nb ? rr * (d[i] - a1 - z[i] * a2) : 0.f;
      __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(o), ro, vo, r * ldb * 4, 0);
    }
    __syncthreads();                  // every wave's red reads before the next tile's writes
  }
}

// Large batches on the matrix cores (GfkModel.lb_fused; round 6).  The library GEMMs above
// read and write the whole [bmax][ldb] logit matrix and run the skinny products (K = 50 inner
// or outer dimension) on tiles built for square ones; these two kernels keep each 64-column
// tile's work inside one workgroup (16 waves, persistent over the tiles, one per CU):
//  * prodlda_lb_fwd (bit 0, bmax 256, K <= 208): the logits of the tile on the fp32
//    matrix cores -- A = theta_d's row tile of the wave, held in registers for the whole
//    persistent loop, B = the tile's beta rows by LDS-DMA (double-buffered; rows >= K and
//    columns past ldb read 0) -- in accumulators (wave w: row tile w x the tile's 4 column
//    strips); then prodlda_lb_colbn's work on the registers:
//    column statistics (the wave's rows + two lane shuffles, the 16 waves through LDS in a
//    fixed order), running statistics / rstd, the BN'ed tile into ws_zn, the per-row sum-exp
//    partials (slot 0 of the workgroup's 4).
//  * prodlda_lb_bwd (bit 1, bmax 256, K <= 208; bit 2: beta's Adam step in its epilogue, the
//    rest of the model in gradient mode + the generic optimizer): prodlda_lb_dlogit's logit
//    gradient into LDS (D [256][68]), beta's tile by LDS-DMA (Bt [16 KT][68], rows >= K zero),
//    then dbeta[k][c] = sum_b theta_d[b][k] D[b][c] (subtiles (k tile, column strip) over the
//    waves, theta_d from L2) into beta's gradient slot, and d theta_d[b][k] += sum_c D[b][c]
//    beta[k][c] (wave w: row tile w x every k tile, accumulated in registers over the
//    workgroup's tiles; one slab per workgroup, n_dpart = the grid, summed by row_bwd).
// Reference: decoder_network.py:121-126 (ProdLDA decoder), avitm.py:84-85 (any batch_size).
constexpr int LBB_LD = 68;                   // LDS row stride of D / Bt (conflict-free A reads)
// Forward: wave w of 8 owns row tiles w and w + 8 (16 rows each) of the 256, their theta_d
// A operands for every k step held in registers for the whole persistent loop (2 KS per lane,
// KS = ceil(K / 4); theta_d is the same for every tile; 8 waves so that K = 200's 104 of them
// fit without spills), and the tile's beta rows come by LDS-DMA into one of two
// buffers (Bs [4 ceil(K / 4)][LBF_LD], rows >= K zeroed once: the next tile's rows land while
// this one multiplies), read as the MFMA B operand (4 rows x 16 columns per instruction at
// stride 80: 64 distinct banks).
constexpr int LBF_LD = 80;
constexpr int LBF_NT = 512;                  // 8 waves (one workgroup per CU: up to 256 VGPRs)
// (rows padded to whole 4-k MFMA steps: the steps read rows K .. 4 ceil(K / 4) - 1 as B operands)
__host__ __device__ inline int lb_fwd_lds_floats(int K) { return 2 * ((K + 3) / 4 * 4) * LBF_LD; }
template <int KS>
__global__ void __launch_bounds__(LBF_NT) prodlda_lb_fwd_kernel(GfkArgT<false> ga) {
  constexpr int BM = 256, NW = LBF_NT / 64, RTW = BM / 16 / NW;
  const GfkModel& m = gfk_model(ga);
  extern __shared__ __attribute__((aligned(16))) float smem[];
  __shared__ float red[2][NW][VB];
  const int tid = threadIdx.x, lane = tid & 63, w = uniform(tid >> 6);
  const int r16 = lane & 15, g = lane >> 4;
  const int K = m.K, V = m.V, ldb = m.ldb, kt = m.kt, nb = *m.ws_nb;
  const int nks = (K + 3) / 4;
  const float inv_nb = 1.f / (float)nb;
  float* bs0 = smem;
  float* bs1 = smem + 4 * nks * LBF_LD;
  // rows K .. 4 nks - 1 of both buffers: the last k step multiplies them by theta_d's zero
  // padding, and 0 x (whatever an earlier kernel left in LDS, a NaN or Inf at times) is NaN.
  // The DMA never writes them: zeroed once (the loop's first barrier orders the stores)
  for (int i = tid; i < (4 * nks - K) * LBF_LD; i += LBF_NT) {
    bs0[K * LBF_LD + i] = 0.f;
    bs1[K * LBF_LD + i] = 0.f;
  }
  const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc((void*)m.beta, 0, K * ldb * 4, 0x00020000);
  if (gfk_bx() == 0 && tid == 0) *m.nbt_beta += 1;
  // beta's rows of a tile -> LDS: wave w copies rows w + NW u (64 columns; past ldb: zeros)
  auto dma = [&](int tile, float* buf) {
    const int c = tile * VB + lane;
    const int vb = c < ldb ? c * 4 : 0x7FFF0000;
    for (int k = w; k < K; k += NW)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rb, (lds_void_ptr)(buf + k * LBF_LD), 4, boff(vb, k * ldb * 4), 0, 0, 0);
  };
  if (gfk_bx() < m.n_tiles) dma(gfk_bx(), bs0);
  // A[i][kk] = theta_d[16 (w + NW j) + i][4 s + kk]: lane (r16, g) holds it in th[j][s]
  float th[RTW][KS];
#pragma unroll
  for (int j = 0; j < RTW; ++j) {
    const float* tr = m.ws_thetad + (size_t)(16 * (w + NW * j) + r16) * kt;
#pragma unroll
    for (int q = 0; q < KS; ++q) th[j][q] = tr[min(4 * q + g, K - 1)] * (4 * q + g < K ? 1.f : 0.f);
  }
  float rs[RTW][4];
#pragma unroll
  for (int j = 0; j < RTW; ++j)
#pragma unroll
    for (int e = 0; e < 4; ++e) rs[j][e] = 0.f;
  int it = 0;
#pragma unroll 1
  for (int tile = gfk_bx(); tile < m.n_tiles; tile += gridDim.x, ++it) {
    const int c0 = tile * VB;
    float* bcur = (it & 1) ? bs1 : bs0;
    float rm0[4], rv0[4];
    if (w == 0) {
#pragma unroll
      for (int cs = 0; cs < 4; ++cs) {
        const int vc = min(c0 + 16 * cs + r16, V - 1);
        rm0[cs] = m.beta_rm[vc];
        rv0[cs] = m.beta_rv[vc];
      }
    }
    GFK_STAMP(m, 130);
    vm_barrier();                            // this tile's beta rows (and every older access)
    GFK_STAMP(m, 131);
    if (tile + (int)gridDim.x < m.n_tiles) dma(tile + gridDim.x, (it & 1) ? bs0 : bs1);
    f32x4 acc[RTW][4];
#pragma unroll
    for (int j = 0; j < RTW; ++j)
#pragma unroll
      for (int cs = 0; cs < 4; ++cs) acc[j][cs] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float* bp = bcur + g * LBF_LD + r16;
#pragma unroll
    for (int q = 0; q < KS; ++q) {
      if (q < nks) {
#pragma unroll
        for (int cs = 0; cs < 4; ++cs) {
          const float bv = bp[4 * q * LBF_LD + 16 * cs];
#pragma unroll
          for (int j = 0; j < RTW; ++j) acc[j][cs] = mfma16x16x4(th[j][q], bv, acc[j][cs]);
        }
      }
      // (a scheduling fence every 4 steps: the B reads stay near their MFMAs instead of all
      // being hoisted into registers next to the resident theta_d operands)
      if ((q & 3) == 3) __builtin_amdgcn_sched_barrier(0);
    }
    GFK_STAMP(m, 132);
    // ---- column statistics over the batch rows (rows >= nb excluded), two-pass variance ----
    float mean[4], rstd[4], sv[4];
#pragma unroll
    for (int cs = 0; cs < 4; ++cs) {
      float v = 0.f;
#pragma unroll
      for (int j = 0; j < RTW; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) v += 16 * (w + NW * j) + 4 * g + e < nb ? acc[j][cs][e] : 0.f;
      v += __shfl_xor(v, 16);
      sv[cs] = v + __shfl_xor(v, 32);
    }
    if (g == 0) {
#pragma unroll
      for (int cs = 0; cs < 4; ++cs) red[0][w][16 * cs + r16] = sv[cs];
    }
    __syncthreads();
#pragma unroll
    for (int cs = 0; cs < 4; ++cs) {
      float mu = 0.f;
#pragma unroll
      for (int q = 0; q < NW; ++q) mu += red[0][q][16 * cs + r16];
      mean[cs] = mu * inv_nb;
      float v = 0.f;
#pragma unroll
      for (int j = 0; j < RTW; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float d = acc[j][cs][e] - mean[cs];
          v += 16 * (w + NW * j) + 4 * g + e < nb ? d * d : 0.f;
        }
      v += __shfl_xor(v, 16);
      sv[cs] = v + __shfl_xor(v, 32);
    }
    if (g == 0) {
#pragma unroll
      for (int cs = 0; cs < 4; ++cs) red[1][w][16 * cs + r16] = sv[cs];
    }
    __syncthreads();
#pragma unroll
    for (int cs = 0; cs < 4; ++cs) {
      float var = 0.f;
#pragma unroll
      for (int q = 0; q < NW; ++q) var += red[1][q][16 * cs + r16];
      var *= inv_nb;
      rstd[cs] = rsqrtf(var + m.bn_eps);
      const int v = c0 + 16 * cs + r16;
      if (w == 0 && g == 0 && v < V) {
        const float mom = m.bn_momentum;
        const float unb = nb > 1 ? var * (float)nb / (float)(nb - 1) : var;
        float nm = (1.f - mom) * rm0[cs] + mom * mean[cs], nv = (1.f - mom) * rv0[cs] + mom * unb;
        if (m.fed_scale_on && is_shared(m, m.beta_rm)) { nm *= m.fed_scale; nv *= m.fed_scale; }
        m.beta_rm[v] = nm;
        m.beta_rv[v] = nv;
        m.ws_col_rstd[v] = rstd[cs];
      }
    }
    GFK_STAMP(m, 133);
    // ---- the BN'ed tile into ws_zn (row_loss's layout), the rows' sum-exp ----
    const __amdgpu_buffer_rsrc_t rz = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(m.ws_zn + (size_t)tile * BM * VB), 0, BM * VB * 4, 0x00020000);
#pragma unroll
    for (int j = 0; j < RTW; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int row = 16 * (w + NW * j) + 4 * g + e;
#pragma unroll
        for (int cs = 0; cs < 4; ++cs) {
          const int col = 16 * cs + r16;
          const float z = (acc[j][cs][e] - mean[cs]) * rstd[cs];
          const int zo = row < nb ? (row * VB + (col ^ zswz(row))) * 4 : 0x7FFF0000;
          __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(z), rz, zo, 0, 0);
          rs[j][e] += (row < nb && c0 + col < V) ? __expf(z) : 0.f;
        }
      }
    // (red[0] is rewritten next tile only after every wave passed the second barrier, which
    // follows its reads; red[1]'s reads precede the next tile's first barrier)
  }
  float* part = m.ws_row_part + (size_t)gfk_bx() * 4 * m.bmax * 2;
#pragma unroll
  for (int j = 0; j < RTW; ++j)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float se = row16_sum(rs[j][e]);
      const int row = 16 * (w + NW * j) + 4 * g + e;
      if (r16 < 4 && row < nb) {
        float* p = part + ((size_t)r16 * m.bmax + row) * 2;
        p[0] = 0.f;                     // (max, sum-exp) with max 0: |z| <= sqrt(nb - 1)
        p[1] = r16 == 0 ? se : 0.f;
      }
    }
}

__host__ __device__ inline int lb_bwd_lds_floats(int K) { return (256 + 16 * ((K + 15) / 16)) * LBB_LD; }

template <int KTM, int NW>
__global__ void __launch_bounds__(64 * NW) prodlda_lb_bwd_kernel(GfkArgT<false> ga) {
  // NW waves (16: every wave's row tile of d theta_d in registers, 4-13 k tiles).  8 waves
  // with two row tiles each (256 VGPRs, no spills at K = 200) measured slower: 413 vs 359 us
  // per step at K = 200, V = 112k (the 16-wave instance spills 24 bytes outside its loops)
  constexpr int BM = 256, NR = BM / NW, RTW = 16 / NW;
  constexpr int RB = NW == 8 ? 4 : 8;        // rows per sparse-entry round (registers)
  constexpr int AV = KTM >= 13 ? 8 : 16;     // theta_d operands in flight per dbeta chunk
  const GfkModel& m = gfk_model(ga);
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* D = smem;                           // [BM][LBB_LD] the logit gradient
  float* Bt = D + BM * LBB_LD;               // [16 KT][LBB_LD] beta's tile (rows >= K: 0)
  __shared__ float red[2][NW][VB];
  __shared__ float sx[NW][VB];               // per wave: the current row's sparse x by column
  const int tid = threadIdx.x, lane = tid & 63, w = uniform(tid >> 6);
  const int r16 = lane & 15, g = lane >> 4;
  const int K = m.K, V = m.V, ldb = m.ldb, kt = m.kt, nb = *m.ws_nb, ntp = m.n_tiles + 1;
  const int KT = (K + 15) / 16;
  const float inv_nb = 1.f / (float)nb;
  const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc((void*)m.beta, 0, K * ldb * 4, 0x00020000);
  const __amdgpu_buffer_rsrc_t rgr = __builtin_amdgcn_make_buffer_rsrc((void*)(m.beta + m.off_g), 0, K * ldb * 4, 0x00020000);
  const __amdgpu_buffer_rsrc_t rmo = __builtin_amdgcn_make_buffer_rsrc((void*)(m.beta + m.off_m), 0, K * ldb * 4, 0x00020000);
  const __amdgpu_buffer_rsrc_t rvo = __builtin_amdgcn_make_buffer_rsrc((void*)(m.beta + m.off_v), 0, K * ldb * 4, 0x00020000);
  // lb_fused bit 2: beta's Adam step (+ the FedAvg pre-scale) in this kernel's dbeta epilogue
  // -- p from the staged tile, m / v loaded next to it; the generic optimizer pass skips beta
  const bool adam_here = m.lb_fused & 4;
  const AdamCoef ac = adam_coef(m);
  const bool pre_scale = m.fed_scale_on && is_shared(m, m.beta);
  const float fscale = m.fed_scale;
  sx[w][lane] = 0.f;
  f32x4 dacc[RTW][KTM];                      // d theta_d [row tile w + NW j][k tile]
#pragma unroll
  for (int j = 0; j < RTW; ++j)
#pragma unroll
    for (int q = 0; q < KTM; ++q) dacc[j][q] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
  for (int tile = gfk_bx(); tile < m.n_tiles; tile += gridDim.x) {
    GFK_STAMP(m, 120);
    const int c0 = tile * VB, v = c0 + lane;
    const bool valid = v < V;
    // beta's tile -> Bt by LDS-DMA: wave w copies rows w + NW u (64 columns each)
    {
      const int vb = v < ldb ? v * 4 : 0x7FFF0000;
      for (int k = w; k < 16 * KT; k += NW)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rb, (lds_void_ptr)(Bt + k * LBB_LD), 4, boff(vb, k * ldb * 4), 0, 0, 0);
    }
    const __amdgpu_buffer_rsrc_t rz = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(m.ws_zn + (size_t)tile * BM * VB), 0, BM * VB * 4, 0x00020000);
    const float rsd = m.ws_col_rstd[min(v, V - 1)];
    // one round of independent loads: lane i holds row w + NW i's extent in this tile, lse
    // and S; every z of the thread's rows (kept in registers); then the rows' non-zeros
    // (their addresses depend on the extents: the second round) in blocks of RB rows
    int ex0 = 0, ex1 = 0;
    float lse_l = 0.f, s_l = 0.f;
    if (lane < NR && w + NW * lane < nb) {
      const int rl = w + NW * lane;
      const int32_t* ts = m.ws_tstart + (size_t)rl * ntp + tile;
      ex0 = ts[0];
      ex1 = ts[1];
      lse_l = m.ws_lse[rl];
      s_l = m.ws_s[rl];
    }
    float z[NR], s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < NR; ++i) {
      const int r = w + NW * i;
      z[i] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rz, (lane ^ zswz(r)) * 4, r * VB * 4, 0));
    }
    // ---- the logit gradient (prodlda_lb_dlogit): d = p S - x p / (p + eps), then the
    //      column BN backward; d parked in D, z kept in registers ----
#pragma unroll
    for (int i0 = 0; i0 < NR; i0 += RB) {
      int ci[RB];
      float xi[RB];
#pragma unroll
      for (int i = 0; i < RB; ++i) {
        const int e0 = __builtin_amdgcn_readlane(ex0, i0 + i), n = __builtin_amdgcn_readlane(ex1, i0 + i) - e0;
        ci[i] = -1;
        xi[i] = 0.f;
        if (lane < n) {
          ci[i] = m.indices[e0 + lane] - c0;
          xi[i] = m.values[e0 + lane];
        }
      }
#pragma unroll
      for (int i = 0; i < RB; ++i) {
        const int r = w + NW * (i0 + i);
        float d = 0.f;
        if (r < nb) {                        // (wave-uniform)
          const float lse_r = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(lse_l), i0 + i));
          const float s_r = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(s_l), i0 + i));
          const float p = __expf(z[i0 + i] - lse_r);
          if (ci[i] >= 0) sx[w][ci[i]] = xi[i];
          const float xs = sx[w][lane];
          sx[w][lane] = 0.f;
          const float dd = p * s_r - xs * p / (p + RL_EPS);
          d = valid ? dd : 0.f;
          s1 += d;
          s2 += d * z[i0 + i];
        } else {
          z[i0 + i] = 0.f;
        }
        D[r * LBB_LD + lane] = d;
      }
    }
    GFK_STAMP(m, 121);
    red[0][w][lane] = s1;
    red[1][w][lane] = s2;
    vm_barrier();                            // (+ beta's tile in LDS)
    GFK_STAMP(m, 122);
    float a1 = 0.f, a2 = 0.f;
#pragma unroll
    for (int q = 0; q < NW; ++q) {
      a1 += red[0][q][lane];
      a2 += red[1][q][lane];
    }
    a1 *= inv_nb;
    a2 *= inv_nb;
    const float rr = valid ? rsd : 0.f;
#pragma unroll
    for (int i = 0; i < NR; ++i) {
      const int r = w + NW * i;
      float* dp = D + r * LBB_LD + lane;
      *dp = r < nb ? rr * (*dp - a1 - z[i] * a2) : 0.f;
    }
    lds_barrier();
    GFK_STAMP(m, 123);
    // ---- dbeta[k][c] = sum_b theta_d[b][k] D[b][c] -> beta's gradient slot ----
    // (A[i][kk] = theta_d[b0 + kk][k0 + i], B[kk][jj] = D[b0 + kk][c0' + jj])
    // KTM >= 13 (K > 128): a wave takes whole k tiles with all 4 column strips, so each
    // theta_d operand is loaded once per tile (the (k tile, strip) round-robin loaded it 4
    // times: 0.8 MB of L2 reads per tile at K = 200); smaller K keeps the round-robin (16
    // subtiles at K = 50: one per wave)
    auto store_g = [&](int ktile, int cs, const f32x4& v4) {
      const int cl = 16 * cs + r16, c = c0 + cl;
      if (adam_here) {                       // (columns >= V keep their zeros)
        const int vo = c < V ? c * 4 : 0x7FFF0000;
        float mo[4], vv[4];
        int off[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int k = 16 * ktile + 4 * g + e;
          off[e] = k < K ? boff(vo, k * ldb * 4) : 0x7FFF0000;
          mo[e] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rmo, off[e], 0, 0));
          vv[e] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rvo, off[e], 0, 0));
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int k = 16 * ktile + 4 * g + e;
          float np = adam_update(Bt[k * LBB_LD + cl], v4[e], mo[e], vv[e], ac);
          if (pre_scale) np *= fscale;
          __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(mo[e]), rmo, off[e], 0, 0);
          __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(vv[e]), rvo, off[e], 0, 0);
          __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(np), rb, off[e], 0, 0);
        }
        return;
      }
      const int vo = c < ldb ? c * 4 : 0x7FFF0000;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int k = 16 * ktile + 4 * g + e;
        if (k < K)
          __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v4[e]), rgr, boff(vo, k * ldb * 4), 0, 0);
      }
    };
    if constexpr (KTM >= 13) {
#pragma unroll 1
      for (int ktile = w; ktile < KT; ktile += NW) {
        const float* ta = m.ws_thetad + min(16 * ktile + r16, K - 1);
        const float* db = D + r16;
        f32x4 acc[4];
#pragma unroll
        for (int cs = 0; cs < 4; ++cs) acc[cs] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
        for (int b0 = 0; b0 < BM; b0 += 4 * AV) {
          float av[AV];
#pragma unroll
          for (int q = 0; q < AV; ++q) av[q] = ta[(size_t)(b0 + 4 * q + g) * kt];
#pragma unroll
          for (int q = 0; q < AV; ++q)
#pragma unroll
            for (int cs = 0; cs < 4; ++cs)
              acc[cs] = mfma16x16x4(av[q], db[(b0 + 4 * q + g) * LBB_LD + 16 * cs], acc[cs]);
        }
#pragma unroll
        for (int cs = 0; cs < 4; ++cs) store_g(ktile, cs, acc[cs]);
      }
    } else {
#pragma unroll 1
      for (int sidx = w; sidx < 4 * KT; sidx += NW) {
        const int ktile = sidx >> 2, cs = sidx & 3;
        const float* ta = m.ws_thetad + min(16 * ktile + r16, K - 1);
        const float* db = D + 16 * cs + r16;
        f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
        for (int b0 = 0; b0 < BM; b0 += 4 * AV) {
          float av[AV];
#pragma unroll
          for (int q = 0; q < AV; ++q) av[q] = ta[(size_t)(b0 + 4 * q + g) * kt];
#pragma unroll
          for (int q = 0; q < AV; q += 2) {
            acc0 = mfma16x16x4(av[q], db[(b0 + 4 * q + g) * LBB_LD], acc0);
            acc1 = mfma16x16x4(av[q + 1], db[(b0 + 4 * q + 4 + g) * LBB_LD], acc1);
          }
        }
        store_g(ktile, cs, acc0 + acc1);
      }
    }
    GFK_STAMP(m, 124);
    // ---- d theta_d[b][k] += sum_c D[b][c] beta[k][c]: row tiles w + NW j x every k tile ----
    // (A[i][kk] = D[16 rt + i][c + kk], B[kk][jj] = beta[16 kt + jj][c + kk])
    {
      const float* bb = Bt + r16 * LBB_LD + g;
#pragma unroll
      for (int c = 0; c < VB; c += 4) {
#pragma unroll
        for (int j = 0; j < RTW; ++j) {
          const float a = D[(16 * (w + NW * j) + r16) * LBB_LD + g + c];
#pragma unroll
          for (int q = 0; q < KTM; ++q)
            if (q < KT) dacc[j][q] = mfma16x16x4(a, bb[q * 16 * LBB_LD + c], dacc[j][q]);
        }
      }
    }
    GFK_STAMP(m, 125);
    __syncthreads();                         // D / Bt / red / sx are rewritten by the next tile
    GFK_STAMP(m, 126);
  }
  // ---- this workgroup's d theta_d partial (slab gfk_bx(); row_bwd sums the slabs in order) ----
  float* dpart = m.ws_dthetad + (size_t)gfk_bx() * m.bmax * K;
#pragma unroll
  for (int j = 0; j < RTW; ++j)
#pragma unroll
    for (int q = 0; q < KTM; ++q) {
      const int k = 16 * q + r16;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int row = 16 * (w + NW * j) + 4 * g + e;
        if (q < KT && k < K && row < nb) dpart[(size_t)row * K + k] = dacc[j][q][e];
      }
    }
}

// Backward.  Two launch shapes of one kernel:
//  * KQ = 1 (every vocab tile has its own workgroup of 16 waves -- the K=50 headline --
//    or K <= 48): workgroup g owns tiles g, g + grid, ...;
//  * KQ = 4 (large vocabularies: more tiles than resident workgroups): the topics are
//    split in 4 ranges of 16-row k tiles; workgroup g handles range q = g % 4 of tiles
//    g / 4, g / 4 + grid / 4, ...  A quarter of theta_d / beta / the Adam state per
//    workgroup (8 waves, ~71 KB of LDS at K = 200, B = 64) lets TWO workgroups share a
//    CU, so one computes while the other's staging round is in flight (a software
//    pipeline inside one workgroup was measured first: the prefetch registers of the
//    next tile are loop-carried, and the compiler's in-order vmcnt waits then serialise
//    them with the current tile's Adam state anyway).  The logit-gradient tile (sparse
//    + dense passes, cheap VALU work) is recomputed by the 4 range workgroups of a tile.
// Every global read of a tile is issued in ONE staging round (theta_d's k range, lse
// and S once per workgroup); the Adam state after the first non-zero's dependent load
// (issuing it before that load measured 5 % slower at K = 200, V = 112k).  The d theta_d partial of the k range is accumulated in
// registers over the workgroup's tiles (each element owned by one lane, fixed order:
// deterministic) and stored once into slab g / KQ, so row_bwd reduces n_dpart = grid /
// KQ partials.  p comes from the staged beta tile (LDS); the Adam results go to fresh
// registers and are stored after every update, so no store waits on a load.
// Per tile:
//   sparse  dt[b, c] = -x p / (p + 1e-10) at the tile's non-zeros
//   dense   dt = rstd * (d - mean_b d - z mean_b(d z)),  d = p S + dt  (column BN bwd)
//   dbeta   g[k, c] = sum_b th[b, k] dt[b, c] -> Adam (+ FedAvg pre-scale) or gradient
//   dtheta  acc[b, k] += sum_c dt[b, c] beta[k, c]          (MFMA, registers)
// dynamic LDS: th[BM*KTQ] + bt[KPQ*LDB_B] + zt[BM*VB] + dt[BM*LDD] + lse[BM] + S[BM] + rstd[VB]
//   (KPQ: rows of the k range, 16 * ceil(ceil(K/16) / KQ); KTQ = kt (KQ = 1) or
//   kt_stride(KPQ))
// MAXU = ceil(K / 64) bounds the k tiles (compile time, so the Adam state and the
// accumulators stay in registers).
__host__ __device__ __forceinline__ int kt_stride(int w) { return w % 32 == 16 ? w : w + 16; }
__host__ __device__ __forceinline__ int bwd_kpq(int K, int kq) { return 16 * ((round_up(K, 16) / 16 + kq - 1) / kq); }
// the 8-wave tile backward (stage_flags GFK_BWD_BATCH8): floats of the region that holds the
// logit tile [B][VB] and after it the beta block [KPQ][LDB_B]
__host__ __device__ __forceinline__ int bwd_zb(int B, int KPQ) { return B * VB > KPQ * LDB_B ? B * VB : KPQ * LDB_B; }
// bwd_pre = 3 runs the software-pipelined backward (fp32, B = 64; else the bwd_pre = 2 one),
// whose dlogit tiles are dense [B][64]
// (its buffer-descriptor stores need beta's rows padded to whole 64-column tiles and the
// slot under 2 GB)
__host__ __device__ __forceinline__ bool bwd_pipe(const GfkModel& m) {
  return m.bwd_pre == 3 && m.bmax == 64 && (m.ldb & 63) == 0 &&
         (int64_t)m.K * m.ldb * 4 < 0x7FFF0000LL;
}

// Logit gradient of one vocabulary tile, computed ONCE (bwd_pre: the persistent k-range
// backward at large V, whose 4 range workgroups per tile each recomputed it, each behind
// a dependent tile-start -> first-non-zero load chain):
//   sparse  dt[b, c] = -x p / (p + 1e-10) at the tile's non-zeros  (p = exp(z - lse_b))
//   dense   dt = rstd * (d - mean_b d - z mean_b(d z)),  d = p S_b + dt  (column BN bwd)
// written to ws_dt[tile] in the backward's LDS tile layout ([BM][LDD], rows >= nb and the
// padding columns zero), so prodlda_bwd stages it with one contiguous LDS-DMA copy.
// grid: n_tiles workgroups of 256 threads.  Static LDS: z tile + dt tile + lse / S / rstd.
template <int BM, bool GB = false>
__global__ void __launch_bounds__(256) prodlda_dlogit_kernel(GfkArgT<GB> ga) {
  const GfkModel& m = gfk_model(ga);
  constexpr int NT = 256;
  constexpr int TPR = NT / BM;                 // threads per row (sparse term)
  __shared__ __attribute__((aligned(16))) float zt[BM * VB];
  __shared__ __attribute__((aligned(16))) float dt[BM * LDD];
  __shared__ __attribute__((aligned(16))) float ls[BM], Sb[BM], rs[VB];
  const int tid = threadIdx.x, tile = gfk_bx(), c0 = tile * VB;
  const int V = m.V, nb = *m.ws_nb;
  // ---- one staging round: z tile, lse, S (LDS-DMA), rstd, the rows' tile extents ----
  glds_copy(zt, m.ws_zn + (size_t)tile * BM * VB, BM * VB, tid, NT);
  glds_copy(ls, m.ws_lse, BM, tid, NT);
  glds_copy(Sb, m.ws_s, BM, tid, NT);
  const int xrow = tid / TPR, xsub = tid % TPR;
  const int32_t* ts = m.ws_tstart + (size_t)xrow * (m.n_tiles + 1) + tile;
  const int xe0 = ts[0], xe1 = ts[1];
  const float rsr = m.ws_col_rstd[min(c0 + (tid & (VB - 1)), m.n_tiles * VB - 1)];
  {
    f32x4* d4 = reinterpret_cast<f32x4*>(dt);
    for (int i = tid; i < BM * LDD / 4; i += NT) d4[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  if (tid < VB) rs[tid] = c0 + tid < V ? rsr : 0.f;
  vm_barrier();
  // ---- sparse term at this tile's non-zeros ----
  if (xrow < nb) {
    const float l = ls[xrow];
    for (int e = xe0 + xsub; e < xe1; e += TPR) {
      const int c = m.indices[e] - c0;
      const float x = m.values[e];
      const float p = __expf(zt[xrow * VB + (c ^ zswz(xrow))] - l);
      dt[xrow * LDD + c] = -x * p / (p + RL_EPS);
    }
  }
  lds_barrier();
  // ---- dense term p S and the column BN backward: 16 lanes per column ----
  const int dg = tid & 15;
  const float inv_nb = 1.f / (float)nb;
  for (int dcol = tid >> 4; dcol < VB; dcol += NT / 16) {
    constexpr int NR = BM / 16;
    float d[NR], z[NR];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < NR; ++i) {
      const int row = dg + 16 * i;
      z[i] = zt[row * VB + (dcol ^ zswz(row))];
      const float p = __expf(z[i] - ls[row]);
      d[i] = row < nb ? p * Sb[row] + dt[row * LDD + dcol] : 0.f;
      s1 += d[i];
      s2 += d[i] * z[i];
    }
    s1 = row16_sum(s1) * inv_nb;
    s2 = row16_sum(s2) * inv_nb;
    const float r = rs[dcol];
#pragma unroll
    for (int i = 0; i < NR; ++i) {
      const int row = dg + 16 * i;
      dt[row * LDD + dcol] = row < nb ? r * (d[i] - s1 - z[i] * s2) : 0.f;
    }
  }
  lds_barrier();
  if (bwd_pipe(m)) {
    // ---- dense [BM][64] (the pipelined backward reads it into registers) ----
    f32x4* out = reinterpret_cast<f32x4*>(m.ws_dt + (size_t)tile * BM * VB);
    for (int i = tid; i < BM * VB / 4; i += NT) {
      const float2* s2 = reinterpret_cast<const float2*>(dt + (i >> 4) * LDD + (i & 15) * 4);
      const float2 a = s2[0], b = s2[1];
      out[i] = f32x4{a.x, a.y, b.x, b.y};
    }
    return;
  }
  // ---- the tile, verbatim (float4 over the flat [BM][LDD] block) ----
  f32x4* out = reinterpret_cast<f32x4*>(m.ws_dt + (size_t)tile * BM * LDD);
  const f32x4* d4 = reinterpret_cast<const f32x4*>(dt);
  for (int i = tid; i < BM * LDD / 4; i += NT) out[i] = d4[i];
}

// BF: bf16 MFMA operands (16x16x32 / 16x16x16), fp32 accumulation, for both GEMMs.
// PRE (bwd_pre, KQ = 4 only): the logit-gradient tile comes precomputed from ws_dt
// (prodlda_dlogit): no sparse / dense passes, no dependent loads in the staging round.
// Its LDS is th [BM][64] (theta_d's k range, row r's columns XOR 16 (r & 1): the dbeta
// A-role reads, 2 rows x 16 columns per half-wave, hit 32 distinct banks with the
// swizzle a per-lane constant) + bt + dt, and the dbeta tile G reuses dt's space (one
// extra barrier): ~50 KB at B = 64, K = 200, so THREE workgroups share a CU (24 waves)
// instead of two.
// NT (KQ = 1 only; 0: the 16-wave workgroup): the 8-wave tile backward of the batched
// headline (stage_flags GFK_BWD_BATCH8).  Three workgroups share a CU (80 VGPRs, a third of
// the LDS), so M clients' tiles are all resident where two 16-wave workgroups per CU leave a
// second round.  Its LDS is th + one region for the logit tile and then the beta block
// (the beta block waits in registers through the sparse and dense passes) + dt, which the
// G tile reuses (through registers and one barrier, as PRE does) + lse / S / rstd; the
// row-wise Adam state is loaded after both MFMA blocks.  Every output element keeps the
// 16-wave instance's arithmetic: only the wave or thread that computes it changes.
template <int BM, int MAXU, int KQ, bool BF, bool PRE, bool OWN = false, int NT = 0>
__device__ __forceinline__ void prodlda_bwd_body(const GfkModel& m) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int NTH = NT ? NT : KQ == 1 ? DEC_THREADS : 512;
  constexpr bool CL = NT != 0;                 // the compact LDS layout above
  static_assert(!CL || (KQ == 1 && !PRE && !BF && NT == 512 && BM == 64 && MAXU == 1), "8-wave tile backward");
  // KQ = 1 with more than 3 k tiles only ever runs with one tile per workgroup (the
  // persistent shape of such K is KQ = 4): no tile loop, no loop-carried registers
  constexpr bool SINGLE = KQ == 1 && MAXU >= 2;
  constexpr int NW = NTH / 64;                                  // waves
  constexpr int NKS = (4 * MAXU + KQ - 1) / KQ;                 // max k tiles per range
  constexpr int TPR = NTH / BM < 16 ? NTH / BM : 16;            // threads per row (sparse x)
  constexpr int BU = (NKS * 16 * VB + NTH - 1) / NTH;           // beta floats per thread
  constexpr int MU = (NKS * 4 + NW - 1) / NW;                   // dbeta subtiles per wave
  constexpr int NDT = ((BM / 16) * NKS + NW - 1) / NW;          // d theta_d subtiles per wave
  // RW: the dbeta tile goes through LDS (the logit tile's buffer, free after the dense
  // pass) so the optimizer epilogue reads and writes m / v / beta along rows: every
  // load / store instruction covers 256 contiguous bytes of one row, instead of the MFMA
  // output layout's 4 rows x 64 B (adam_rmw_bandwidth.jsonl: 5.7 vs 4.2 TB/s)
  constexpr bool RW = 16 * NKS <= BM;
  constexpr int RPU = NTH / VB;                                 // block rows per thread slot
  static_assert(NTH % VB == 0 && RPU % 8 == 0, "row-slot layout");
  constexpr int RU = RW ? (16 * NKS * VB + NTH - 1) / NTH : 1;  // row-wise elements per thread
  const int K = m.K, V = m.V;
  // the thread index is re-made opaque at every tile (below), so the compiler rebuilds
  // the lane-dependent addresses inside the tile loop instead of hoisting them all out
  // of it (which would cost tens of VGPRs and spill)
  int tid = threadIdx.x;
  int lane = tid & 63, wave = uniform(tid >> 6);
  const int ksub = round_up(K, 16) / 16;
  const int q = (int)gfk_bx() % KQ, slab = (int)gfk_bx() / KQ, nslab = (int)gridDim.x / KQ;
  const int ks0 = q * ksub / KQ, nks = (q + 1) * ksub / KQ - ks0;   // this workgroup's k tiles
  const int kb = 16 * ks0;                                      // first topic of the range
  const int KPQ = bwd_kpq(K, KQ), KTQ = PRE ? 64 : KQ == 1 ? m.kt : kt_stride(KPQ);
  float* th = smem;
  float* bt = th + BM * KTQ;
  float* zt = CL ? bt : bt + KPQ * LDB_B;       // PRE: no logit tile; the G tile aliases dt
  float* dt = PRE ? zt : CL ? zt + bwd_zb(BM, KPQ) : zt + BM * VB;
  float* lse = dt + BM * LDD;
  float* Sb = lse + BM;
  float* rs = Sb + BM;
  const int NB_T = nks * 4;                    // dbeta subtiles (k tile, column strip)
  const int NDT_T = (BM / 16) * nks;           // d theta_d subtiles (row tile, k tile)
  const bool fused = m.update_mode == 1;
  const int nb = *m.ws_nb;
  const AdamCoef ac = adam_coef(m);
  const bool beta_shared = is_shared(m, m.beta);

  GFK_STAMP(m, 24);
  // batched launches (tools/stamps.py --clients): the first-tile and the last-tile workgroup,
  // slots 600 / 608 + entry, staged, dense done, end
#ifdef GFK_STAMPS
  const bool stamp2 = m.n_batch > 1 && KQ == 1 && (slab == 0 || slab == nslab - 1);
  const int slot2 = slab == 0 ? 600 : 608;
#endif
  GFK_STAMP_IF(m, stamp2, slot2);
  // ---- once per workgroup: theta_d columns [kb, kb + 16 nks), lse, S ----
  if (KQ == 1) {
    glds_copy(th, m.ws_thetad, BM * m.kt, tid, NTH);           // KTQ == kt for one range
  } else {
    for (int i = tid; i < BM * 16 * NKS; i += NTH) {
      const int b = i / (16 * NKS), c = i % (16 * NKS);
      if (PRE) th[b * 64 + (c ^ (((b >> 3) & 1) << 4))] = c < 16 * nks ? m.ws_thetad[(size_t)b * m.kt + kb + c] : 0.f;
      else if (c < 16 * nks) th[b * KTQ + c] = m.ws_thetad[(size_t)b * m.kt + kb + c];
    }
  }
  if (!PRE) {
    glds_copy(lse, m.ws_lse, BM, tid, NTH);
    glds_copy(Sb, m.ws_s, BM, tid, NTH);
  }

  // ---- a tile's loads, into registers ----
  float br[BU];
  float rsr = 0.f;
  int xe0 = 0, xe1 = 0, xc0 = 0;
  float xv0 = 0.f;
  int xrow = tid / TPR, xsub = tid % TPR;
  auto issue_tile = [&](int tile) {
    const int c0 = tile * VB;
    // the tile-start loads first: the dependent first-non-zero load waits for them
    // alone (vmcnt counts in order), not for the beta block behind them
    if (!PRE) {
      const int32_t* ts = m.ws_tstart + (size_t)min(xrow, BM - 1) * (m.n_tiles + 1) + tile;
      xe0 = ts[0];                       // rows >= BM (BM < NTH / 16) are never used
      xe1 = ts[1];
    }
    // element tid + NTH u of the block is (row tid / VB + RPU u, column tid % VB)
    const int c = min(c0 + (tid & (VB - 1)), V - 1);
#pragma unroll
    for (int u = 0; u < BU; ++u) {
      const int k = min(kb + tid / VB + RPU * u, K - 1);
      br[u] = m.beta[k * m.ldb + c];             // 32-bit offsets (K ldb < 2^31)
    }
    if (!PRE) rsr = m.ws_col_rstd[c0 + (tid & (VB - 1))];
  };
  auto issue_first_nz = [&]() {          // depends on the tile-start loads
    const int xe = min(xe0 + xsub, max(xe1 - 1, 0));
    xc0 = m.indices[xe];
    xv0 = m.values[xe];
  };
  // Adam state of this lane's dbeta outputs: subtile t -> (k tile kb/16 + t/4, strip t%4)
  float bm_[MU][4], bv_[MU][4];
  auto issue_state = [&](int tile) {
    const int c0 = tile * VB;
#pragma unroll
    for (int u = 0; u < MU; ++u) {
      const int t = wave + NW * u;
      const int ks = t >> 2, cst = t & 3;
      const int c = min(c0 + cst * 16 + (lane & 15), V - 1);
#pragma unroll
      for (int r = 0; r < 4; ++r) {   // unpredicated, clamped (no select on a pending load)
        const int k = min(kb + ks * 16 + (lane >> 4) * 4 + r, K - 1);
        const float* p = m.beta + (size_t)k * m.ldb + c;
        bm_[u][r] = p[m.off_m];
        bv_[u][r] = p[m.off_v];
      }
    }
  };
  float rm_[RU], rv_[RU];                       // (RW) row-wise Adam state of this thread
  // (RW) the row-wise epilogue's beta / m / v / gradient traffic through buffer descriptors:
  // one column offset per tile (columns past V: an offset outside the descriptor, so loads
  // return 0 and stores are dropped -- beta's rows need no padding here) and a row offset
  // per element; element rows are wave-uniform (row = kb + wave + RPU u), checked by a
  // scalar branch.  Replaces a 64-bit address + bounds branch per element.
  const int nrec = K * m.ldb * 4;               // (K ldb 4 < 0x7FFF0000: the launcher)
  // (rs_b: stores only -- the new beta goes to the client's own copy, gfk_own)
  const __amdgpu_buffer_rsrc_t rs_b = __builtin_amdgcn_make_buffer_rsrc((void*)(m.beta + gfk_own<OWN>(m)), 0, nrec, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_m = __builtin_amdgcn_make_buffer_rsrc((void*)(m.beta + m.off_m), 0, nrec, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_v = __builtin_amdgcn_make_buffer_rsrc((void*)(m.beta + m.off_v), 0, nrec, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_g = __builtin_amdgcn_make_buffer_rsrc((void*)(m.beta + m.off_g), 0, nrec, 0x00020000);
  auto rw_col = [&](int tile) {                 // byte offset of this thread's column
    const int c = tile * VB + (tid & (VB - 1));
    return c < V ? c * 4 : 0x7FFF0000;
  };
  auto issue_state_rw = [&](int tile, float (&sm_)[RU], float (&sv_)[RU]) {
    const int vcol = rw_col(tile);
#pragma unroll
    for (int u = 0; u < RU; ++u) {
      const int k = min(kb + tid / VB + RPU * u, K - 1);
      const int vo = boff(vcol, k * m.ldb * 4);
      sm_[u] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs_m, vo, 0, 0));
      sv_[u] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs_v, vo, 0, 0));
    }
  };
  // this workgroup's d theta_d partial, per lane (summed over its tiles in order)
  f32x4 dacc[NDT];
#pragma unroll
  for (int j = 0; j < NDT; ++j) dacc[j] = f32x4{0.f, 0.f, 0.f, 0.f};

  int tile = slab;
  const int dg = threadIdx.x & 15;             // dense-pass layout: row group (16 lanes per column)
#pragma unroll 1
  for (; tile < m.n_tiles; tile += nslab) {
    const int c0 = tile * VB;
    asm volatile("" : "+v"(tid));
    __builtin_assume(tid >= 0 && tid < NTH);   // (unsigned index math after the opaque asm)
    lane = tid & 63;
    wave = uniform(tid >> 6);
    xrow = tid / TPR;
    xsub = tid % TPR;
    GFK_STAMP(m, 23);
    // one staging round per tile: every global read is issued before the barrier
    issue_tile(tile);
    if (!PRE) issue_first_nz();
    if (fused && !CL) {
      if constexpr (RW) issue_state_rw(tile, rm_, rv_);
      else issue_state(tile);
    }
    if (tile != slab) lds_barrier();           // the previous tile's LDS reads are done
    // ---- (1) the BN'ed logit tile by LDS-DMA (contiguous in ws_zn), this tile's
    //      registers -> LDS; zero the logit-gradient tile ----
    if (PRE) glds_copy(dt, m.ws_dt + (size_t)tile * BM * LDD, BM * LDD, tid, NTH);
    else glds_copy(zt, m.ws_zn + (size_t)tile * BM * VB, BM * VB, tid, NTH);
    if constexpr (!CL) {
      const int c = tid & (VB - 1), cok = c0 + c < V;
#pragma unroll
      for (int u = 0; u < BU; ++u) {
        const int k = tid / VB + RPU * u;
        if (k < 16 * nks) bt[k * LDB_B + c] = (kb + k < K && cok) ? br[u] : 0.f;
      }
    }
    if (!PRE) {
      if (tid < VB) rs[tid] = rsr;
      for (int dcol = tid >> 4; dcol < VB; dcol += NTH / 16)
        for (int row = dg; row < BM; row += 16) dt[row * LDD + dcol] = 0.f;
    }
    const int ye0 = xe0, ye1 = xe1, yc0 = xc0;
    const float yv0 = xv0;
    vm_barrier();                              // (+ theta_d / lse / S on the first tile)
    // the same wait, visible to the compiler's waitcnt pass (it cannot see inside the
    // asm): every load of the staging round is now known complete, so no later use of
    // the Adam state waits on the epilogue's own stores (vmcnt counts stores too)
    __builtin_amdgcn_s_waitcnt(0x0F70);        // vmcnt(0) expcnt(7) lgkmcnt(15)
    GFK_STAMP(m, 25);
    GFK_STAMP_IF(m, stamp2, slot2 + 1);

    // ---- (3) sparse term: dt[b, c] = -x p / (p + 1e-10) at this tile's non-zeros ----
    if (!PRE) {
    if (xrow < nb && xrow < BM) {
      const float l = lse[xrow];
      for (int i = 0, e = ye0 + xsub; e < ye1; ++i, e += TPR) {
        const int c = (i == 0 ? yc0 : m.indices[e]) - c0;
        const float x = i == 0 ? yv0 : m.values[e];
        const float p = __expf(zt[xrow * VB + (c ^ zswz(xrow))] - l);
        dt[xrow * LDD + c] = -x * p / (p + RL_EPS);
      }
    }
    lds_barrier();
    GFK_STAMP(m, 26);

    // ---- (4) dense term p*S and the column BN backward: 16 lanes per column ----
    for (int dcol = tid >> 4; dcol < VB; dcol += NTH / 16) {
      const bool valid = c0 + dcol < V;
      constexpr int NR = BM / 16;
      float d[NR], z[NR];
      float s1 = 0.f, s2 = 0.f;
#pragma unroll
      for (int i = 0; i < NR; ++i) {
        const int row = dg + 16 * i;
        z[i] = zt[row * VB + (dcol ^ zswz(row))];
        const float p = __expf(z[i] - lse[row]);
        d[i] = (row < nb && valid) ? p * Sb[row] + dt[row * LDD + dcol] : 0.f;
        s1 += d[i];
        s2 += d[i] * z[i];
      }
      s1 = row16_sum(s1) / (float)nb;
      s2 = row16_sum(s2) / (float)nb;
      const float r = valid ? rs[dcol] : 0.f;
#pragma unroll
      for (int i = 0; i < NR; ++i) {
        const int row = dg + 16 * i;
        dt[row * LDD + dcol] = row < nb ? r * (d[i] - s1 - z[i] * s2) : 0.f;
      }
    }
    lds_barrier();
    }  // !PRE
    GFK_STAMP(m, 27);
    GFK_STAMP_IF(m, stamp2, slot2 + 2);
    if constexpr (CL) {         // the logit tile is done: its region takes the beta block
      const int c = tid & (VB - 1), cok = c0 + c < V;
#pragma unroll
      for (int u = 0; u < BU; ++u) {
        const int k = tid / VB + RPU * u;
        if (k < 16 * nks) bt[k * LDB_B + c] = (kb + k < K && cok) ? br[u] : 0.f;
      }
      lds_barrier();
    }

    // ---- (5) d theta_d[b, k] += sum_c dlogit[b, c] beta[k, c] over the k range ----
    auto dtheta_tile = [&]() {
#pragma unroll
    for (int j = 0; j < NDT; ++j) {
      const int t = wave + NW * j;
      if (t >= NDT_T) break;
      const int rt = t / nks, ks = t % nks;
      if constexpr (BF) {         // A[b][c] = dt row, B[c][k] = beta row: 8 consecutive c each
        const float* ap = dt + (rt * 16 + (lane & 15)) * LDD + 8 * (lane >> 4);
        const float* bp = bt + (ks * 16 + (lane & 15)) * LDB_B + 8 * (lane >> 4);
        f32x4 a0 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < VB; c += 32) {
          float a[8], b[8];
#pragma unroll
          for (int q = 0; q < 8; ++q) { a[q] = ap[c + q]; b[q] = bp[c + q]; }
          a0 = mfma16x16x32bf(a, b, a0);
        }
        dacc[j] += a0;
      } else {
        const float* ap = dt + (rt * 16 + (lane & 15)) * LDD + (lane >> 4);
        const float* bp = bt + (ks * 16 + (lane & 15)) * LDB_B + (lane >> 4);
        f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < VB; c += 8) {
          a0 = mfma16x16x4(ap[c], bp[c], a0);
          a1 = mfma16x16x4(ap[c + 4], bp[c + 4], a1);
        }
        dacc[j] += a0 + a1;
      }
    }
    };
    // ---- (6) dbeta[k, c] = sum_b th[b, k] dlogit[b, c] -> update (fused) or gradient ----
    float gr[MU][4];                           // (PRE: the dbeta subtiles, until G is free)
    auto dbeta_tile = [&]() {
      // results in fresh registers: the stores below never wait on a load (the loaded
      // m, v are consumed only by the fused-mode update)
      float np_[MU][4], mo_[MU][4], vo_[MU][4];
#pragma unroll
      for (int u = 0; u < MU; ++u) {
        const int t = wave + NW * u;
        if (t >= NB_T) break;
        const int ks = t >> 2, cst = t & 3;
        f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
        if constexpr (BF) {       // A[k][b] = theta_d column, B[b][c] = dt column
          if constexpr (BM % 32 == 0) {
            // 8 rows b each: rows 8 g + b0 + q, b0 a multiple of 32 (PRE: swizzle 16 (g & 1))
            const float* ap = th + 8 * (lane >> 4) * KTQ +
                              (PRE ? (ks * 16 + (lane & 15)) ^ (((lane >> 4) & 1) << 4)
                                   : ks * 16 + (lane & 15));
            const float* bp = dt + 8 * (lane >> 4) * LDD + cst * 16 + (lane & 15);
#pragma unroll
            for (int b0 = 0; b0 < BM; b0 += 32) {
              float a[8], b[8];
#pragma unroll
              for (int q = 0; q < 8; ++q) {
                a[q] = ap[(b0 + q) * KTQ];
                b[q] = bp[(b0 + q) * LDD];
              }
              a0 = mfma16x16x32bf(a, b, a0);
            }
          } else {
            // 4 rows b each: rows 4 g + b0 + q, b0 a multiple of 16 (PRE: 16 ((g >> 1) & 1))
            const float* ap = th + 4 * (lane >> 4) * KTQ +
                              (PRE ? (ks * 16 + (lane & 15)) ^ ((((lane >> 4) >> 1) & 1) << 4)
                                   : ks * 16 + (lane & 15));
            const float* bp = dt + 4 * (lane >> 4) * LDD + cst * 16 + (lane & 15);
#pragma unroll
            for (int b0 = 0; b0 < BM; b0 += 16) {
              float a[4], b[4];
#pragma unroll
              for (int q = 0; q < 4; ++q) {
                a[q] = ap[(b0 + q) * KTQ];
                b[q] = bp[(b0 + q) * LDD];
              }
              a0 = mfma16x16x16bf(a, b, a0);
            }
          }
        } else {
          // The batch index b is the MFMA's reduction axis, so any bijection of b over
          // the (step, lane group) pairs works if A and B agree.  Step j, lane group g takes
          // b = 8 g + (j & 7) + 32 (j >> 3) (B >= 32): a half-wave reads rows r and r + 8,
          // whose 16-column runs sit 8 LDD = 528 = 16 (mod 32) banks apart in dt (and
          // 8 KTQ apart in theta_d: 16 mod 32 for the K = 50 stride 50) -- the consecutive
          // rows of the plain mapping (offset LDD = 2 mod 32) overlapped on 14 banks.
          // (PRE: theta_d rows XOR 16 ((b >> 3) & 1) = 16 (g & 1): fixed per lane.)
          constexpr bool R8 = BM >= 32;
          const int g = lane >> 4;
          const int gr = R8 ? 8 * g : g;
          const int kc = ks * 16 + (lane & 15);
          const float* ap = th + gr * KTQ + (PRE && R8 ? kc ^ ((g & 1) << 4) : kc);
          const float* bp = dt + gr * LDD + cst * 16 + (lane & 15);
          // theta_d operand of row r (relative to gr); B = 16 with PRE: per-row swizzle
          auto tha = [&](int r) {
            if (PRE && !R8) return th[(gr + r) * KTQ + (kc ^ ((((gr + r) >> 3) & 1) << 4))];
            return ap[r * KTQ];
          };
#pragma unroll
          for (int j = 0; j < BM / 4; j += 2) {
            const int r0 = R8 ? (j & 7) + 32 * (j >> 3) : 4 * j;
            const int r1 = R8 ? ((j + 1) & 7) + 32 * ((j + 1) >> 3) : 4 * j + 4;
            a0 = mfma16x16x4(tha(r0), bp[r0 * LDD], a0);
            a1 = mfma16x16x4(tha(r1), bp[r1 * LDD], a1);
          }
        }
        const int cl = cst * 16 + (lane & 15);
        if constexpr (RW) {       // into the G tile: row kl at columns XOR 16 (kl & 4), so a
#pragma unroll                    // half-wave's 2 rows x 16 columns hit 32 distinct banks
          for (int e = 0; e < 4; ++e) {
            const int kl = ks * 16 + (lane >> 4) * 4 + e;
            if (PRE || CL) gr[u][e] = a0[e] + a1[e];    // (G aliases dt: stored after a barrier)
            else zt[kl * VB + (cl ^ ((kl & 4) << 2))] = a0[e] + a1[e];
          }
          continue;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float g = a0[e] + a1[e];
          np_[u][e] = mo_[u][e] = vo_[u][e] = g;
          if (fused) {
            const int kl = ks * 16 + (lane >> 4) * 4 + e;
            float mo = bm_[u][e], vo = bv_[u][e];
            float np = adam_update(bt[kl * LDB_B + cl], g, mo, vo, ac);
            np_[u][e] = beta_shared && m.fed_scale_on ? np * m.fed_scale : np;
            mo_[u][e] = mo;
            vo_[u][e] = vo;
          }
        }
      }
      if constexpr (RW) return;
      // every store after every update: no load is pending between them
#pragma unroll
      for (int u = 0; u < MU; ++u) {
        const int t = wave + NW * u;
        if (t >= NB_T) break;
        const int ks = t >> 2, cst = t & 3;
        const int c = c0 + cst * 16 + (lane & 15);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int k = kb + ks * 16 + (lane >> 4) * 4 + e;
          if (k >= K || c >= V) continue;
          float* p = m.beta + (size_t)k * m.ldb + c;
          if (!fused) {
            p[m.off_g] = np_[u][e];
          } else {
            p[m.off_m] = mo_[u][e];
            p[m.off_v] = vo_[u][e];
            p[gfk_own<OWN>(m)] = np_[u][e];
          }
        }
      }
    };
    float tm_[RU] = {}, tv_[RU] = {};          // (CL) this tile's row-wise Adam state
    if ((PRE || CL) && RW) {
      // d theta_d first, then dbeta into registers; every wave is done reading dt before
      // the G tile overwrites it
      dtheta_tile();
      dbeta_tile();
      // (CL) the Adam state behind both MFMA blocks, in registers of this tile's own (rm_ /
      // rv_ live across the tile loop): under them it does not fit 80 VGPRs.  The two
      // barriers of the G tile and the CU's other workgroups cover the loads.
      if constexpr (CL) if (fused) issue_state_rw(tile, tm_, tv_);
      lds_barrier();
#pragma unroll
      for (int u = 0; u < MU; ++u) {
        const int t = wave + NW * u;
        if (t >= NB_T) break;
        const int ks = t >> 2, cl = (t & 3) * 16 + (lane & 15);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int kl = ks * 16 + (lane >> 4) * 4 + e;
          (CL ? dt : zt)[kl * VB + (cl ^ ((kl & 4) << 2))] = gr[u][e];
        }
      }
    } else {
      // (6) first: the Adam state's registers are free before the accumulators are touched
      dbeta_tile();
      dtheta_tile();
    }
    if constexpr (RW) {       // the G tile, row-wise: update (fused) or gradient
      lds_barrier();
      // per thread: one column, rows kl0 + RPU u (RPU a multiple of 8, so the row's
      // XOR swizzle is the same for all u); the row pointer advances by RPU rows
      const int cl = tid & (VB - 1), kl0 = tid / VB;
      const int cs = cl ^ ((kl0 & 4) << 2);
      const int vcol = rw_col(tile);
#pragma unroll
      for (int u = 0; u < RU; ++u) {
        const int kl = kl0 + RPU * u, k = kb + kl;
        if (kl >= 16 * nks || k >= K) continue;   // (wave-uniform)
        const float g = (CL ? dt : zt)[kl * VB + cs];   // the G tile
        const int off = boff(vcol, k * m.ldb * 4);
        if (!fused) {
          __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(g), rs_g, off, 0, 0);
        } else {
          float mo = CL ? tm_[u] : rm_[u], vo = CL ? tv_[u] : rv_[u];
          float np = adam_update(bt[kl * LDB_B + cl], g, mo, vo, ac);
          if (beta_shared && m.fed_scale_on) np *= m.fed_scale;
          __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(mo), rs_m, off, 0, 0);
          __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(vo), rs_v, off, 0, 0);
          __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(np), rs_b, off, 0, 0);
        }
      }
    }
    GFK_STAMP(m, 28);
    GFK_STAMP_IF(m, stamp2, slot2 + 3);
    if (SINGLE) break;
  }
  // ---- this workgroup's d theta_d partial (plain stores; row_bwd sums the slabs in order) ----
  float* dpart = m.ws_dthetad + (size_t)slab * m.bmax * K;
#pragma unroll
  for (int j = 0; j < NDT; ++j) {
    const int t = wave + NW * j;
    if (t >= NDT_T) break;
    const int rt = t / nks, ks = t % nks;
    const int k = kb + ks * 16 + (lane & 15);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int row = rt * 16 + (lane >> 4) * 4 + e;
      if (row < nb && k < K) dpart[(size_t)row * K + k] = dacc[j][e];
    }
  }
}

template <int BM, int MAXU, int KQ, bool BF, bool GB = false>
__global__ void __launch_bounds__(KQ == 1 ? DEC_THREADS : 512, KQ == 1 ? 1 : 2)
prodlda_bwd_kernel(GfkArgT<GB> ga) {
  const GfkModel& m = gfk_model(ga);
  prodlda_bwd_body<BM, MAXU, KQ, BF, false, GB>(m);
}

// stage_flags GFK_BWD_BATCH8: the one-range tile backward in 8 waves (B = 64, K <= 64, fp32),
// three workgroups per CU: 80 VGPRs and at most a third of the LDS (bwd8_ok)
template <int BM, int MAXU, bool GB = false>
__global__ void __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(6)))
prodlda_bwd8_kernel(GfkArgT<GB> ga) {
  const GfkModel& m = gfk_model(ga);
  prodlda_bwd_body<BM, MAXU, 1, false, false, GB, 512>(m);
}

// the precomputed-dlogit shape (bwd_pre = 2): the compiler's register budget, two 8-wave
// workgroups per CU (round 6 removed the 80-VGPR three-per-CU shape, measured slower)
template <int BM, int MAXU, bool BF, bool GB = false>
__global__ void __launch_bounds__(512, 2) prodlda_bwd_pre2_kernel(GfkArgT<GB> ga) {
  const GfkModel& m = gfk_model(ga);
  prodlda_bwd_body<BM, MAXU, 4, BF, true>(m);
}

// bwd_pre = 3: the precomputed-dlogit k-range backward, SOFTWARE-PIPELINED (fp32, B = 64).
// The bwd_pre = 2 kernel waits for a tile's loads, computes, stores, and only then issues
// the next tile's loads: each workgroup's memory traffic stops during its compute, and with
// two workgroups per CU the chip moved ~3.8 TB/s (k200v112k_pre2_sparsewin_counters.md:
// 41 % of wave cycles waiting on memory).  Here, per tile t:
//   top      stage t's beta slice and dlogit tile (registers, loaded during tile t - 1) to LDS
//            issue tile t + nslab's beta slice, dlogit tile and Adam m / v (the latter into
//            the second of two m / v register sets: t's were loaded during tile t - 1)
//   compute  d theta_d / dbeta MFMAs, the G tile, the Adam epilogue and stores
// so every load has a whole tile of compute to arrive (g13 diagnostics: with t's m / v
// issued at the top of tile t, their latency alone held the loop at 117 us without any
// stores), with 32 extra VGPRs (K = 200) and no
// LDS-DMA (whose pending copies make the compiler's vmcnt bookkeeping fall back to
// vmcnt(0)): every wait is the compiler's own.  The dlogit tiles come dense ([B][64],
// written so by prodlda_dlogit).  The 4 range workgroups of a slab sit on ONE XCD
// (blockIdx -> XCD round-robin), so a tile's dlogit block is fetched from HBM once and
// served to the other three from that XCD's L2.
// MFMA operands: both products reduce over a 64-long axis, and the reduction index of MFMA
// step 4 q + j for lane group g is 16 q + 4 g + j (a bijection, the same for A and B), so a
// lane's operands for 4 steps are ONE ds_read_b128 along a row.  Each operand therefore
// lives in LDS with the reduction axis contiguous (row stride 72 floats: 16-byte aligned,
// and every 16-lane ds_read_b128 group of these reads hits distinct banks):
//   d theta_d[b, k] = sum_c dt[b][c] bt[k][c]       (dt: [b][c], bt: [k][c])
//   dbeta[k, c]    = sum_b thT[k][b] dtT[c][b]      (theta_d and dlogit staged transposed)
// -- 8 b128 reads per 16 MFMAs, all issued ahead of them, instead of 16 ds_read2_b32 one
// step ahead (whose LDS latency stalled every MFMA pair: s_waitcnt lgkmcnt(0) each).
// dtT is written transposed from the row-major registers (16 lanes: one b, 16 c rows):
// its columns are XORed with 4 ((c >> 2) & 7), which cuts those ds_write_b32 from 8-way to
// 2-way bank conflicts and keeps the b128 reads conflict-free.
// LDS: thT, bt, dt, dtT: 4 x [64][72] floats (74 KB; the G tile aliases dtT).
constexpr int LDP = 72;
typedef unsigned int gfk_u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ int dtt_swz(int c) { return ((c >> 2) & 7) << 2; }
// Memory operations: beta / m / v / the gradient through buffer descriptors, one 16-byte
// quad per instruction (r4; r3 moved one float per lane: 4x the memory instructions), a
// column offset per tile and per-quad row offsets, instead of a 64-bit address per element
// and a select between the element and a sink: rows past K (the last k range's padding) get
// an out-of-range voffset
// (the descriptor's range check: loads return 0, stores are dropped); columns past V
// fall into beta's row padding (ldb is a multiple of 64 on this path; padding columns have
// a zero gradient and stay zero).  FUSED (Adam + pre-scale, else the gradient) is a
// template parameter: no per-element mode selects.
template <int BM, int MAXU, bool FUSED, bool GB = false>
__global__ void __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4)))
prodlda_bwd_pipe_kernel(GfkArgT<GB> ga) {
  static_assert(BM == 64, "pipelined backward: B = 64");
  const GfkModel& m = gfk_model(ga);
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int NTH = 512, NW = NTH / 64, KQ = 4;
  constexpr int NKS = MAXU;                                    // max k tiles per range
  constexpr int RPU = NTH / VB;                                // 8 block rows per slot
  constexpr int RU = 16 * NKS * VB / NTH;                      // block elements per thread
  constexpr int RQ = (NKS + 1) / 2;                            // ... as quads (4 columns; rows
                                                               //  past 16 NKS: out of range)
  constexpr int RPQ = NTH / (VB / 4);                          // 32 block rows per quad slot
  constexpr int MU = (NKS * 4 + NW - 1) / NW;                  // dbeta subtiles per wave
  constexpr int NDT = ((BM / 16) * NKS + NW - 1) / NW;         // d theta_d subtiles per wave
  constexpr int DU = BM * VB / 4 / NTH;                        // dlogit float4 per thread
  constexpr bool KEEP = FUSED && MAXU <= 2;                    // (register budget: K <= 128)
  const int K = m.K, V = m.V;
  int tid = threadIdx.x;
  int lane = tid & 63, wave = uniform(tid >> 6);
  const int ksub = round_up(K, 16) / 16;
  const int G = (int)gridDim.x, nslab = G / KQ;
  int q, slab;
  if ((G & 31) == 0) {             // XCD-aware: blockIdx b runs on XCD b % 8
    const int b = (int)gfk_bx(), j = b >> 3;
    q = j & 3;
    slab = ((j >> 2) << 3) | (b & 7);
  } else {
    q = (int)gfk_bx() % KQ;
    slab = (int)gfk_bx() / KQ;
  }
  const int ks0 = q * ksub / KQ, nks = (q + 1) * ksub / KQ - ks0;
  const int kb = 16 * ks0;
  float* thT = smem;                            // [64 k][LDP]   theta_d^T of the k range
  float* bt = thT + 64 * LDP;                   // [64 k][LDP]   beta slice
  float* dt = bt + 64 * LDP;                    // [64 b][LDP]   dlogit
  float* dtT = dt + 64 * LDP;                   // [64 c][LDP ^ swz] dlogit^T (then the G tile)
  const int NB_T = nks * 4, NDT_T = (BM / 16) * nks;
  const int nb = *m.ws_nb;
  const AdamCoef ac = adam_coef(m);
  const bool beta_shared = is_shared(m, m.beta);
  const int n_tiles = m.n_tiles;

  for (int i = tid; i < BM * 64; i += NTH) {   // (k >= the range: zero)
    const int b = i >> 6, c = i & 63;
    thT[c * LDP + b] = c < 16 * nks ? m.ws_thetad[(size_t)b * m.kt + kb + c] : 0.f;
  }

  f32x4 br[RQ];
  f32x4 dr[DU];
  // buffer descriptors over beta's slot and its m / v / gradient twins (host-checked:
  // K ldb 4 < 2^31), the dlogit tiles, and the row offsets of this thread's quads
  const int nrec = K * m.ldb * 4;
  const __amdgpu_buffer_rsrc_t rs_b = __builtin_amdgcn_make_buffer_rsrc((void*)m.beta, 0, nrec, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_m = __builtin_amdgcn_make_buffer_rsrc((void*)(m.beta + (FUSED ? m.off_m : m.off_g)), 0, nrec, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_v = __builtin_amdgcn_make_buffer_rsrc((void*)(m.beta + m.off_v), 0, nrec, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_d = __builtin_amdgcn_make_buffer_rsrc((void*)m.ws_dt, 0, n_tiles * BM * VB * 4, 0x00020000);
  // quad u of a thread: block row tid / 16 + 32 u, columns 4 (tid % 16) .. + 3 -- every
  // beta / m / v load and store moves 16 bytes (a wave covers 4 rows x 256 B) instead of 4
  // (one row x 256 B per instruction: 4x the memory instructions for the same bytes)
  int rowoff[RQ];                              // bytes; rows outside the range / K: out of range
#pragma unroll
  for (int u = 0; u < RQ; ++u) {
    const int kl = (tid >> 4) + RPQ * u, k = kb + kl;
    rowoff[u] = kl < 16 * nks && k < K ? k * m.ldb * 4 : 0x7FFF0000;
  }
  const int lane16 = 16 * (tid & 15);
  auto issue_bd = [&](int tile) {             // beta slice + dlogit tile
    const int vc = tile * VB * 4 + lane16;
#pragma unroll
    for (int j = 0; j < DU; ++j) {
      const gfk_u32x4 x = __builtin_amdgcn_raw_buffer_load_b128(rs_d, (tid + NTH * j) * 16, uniform(tile * BM * VB * 4), 0);
      dr[j] = f32x4{__uint_as_float(x.x), __uint_as_float(x.y), __uint_as_float(x.z), __uint_as_float(x.w)};
    }
#pragma unroll
    for (int u = 0; u < RQ; ++u)
      br[u] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_b, boff(vc, rowoff[u]), 0, 0));
  };
  // Adam state (fused mode only)
  auto issue_mv = [&](int tile, f32x4 (&rm)[RQ], f32x4 (&rv)[RQ]) __attribute__((always_inline)) {
    if constexpr (FUSED) {
      const int vc = tile * VB * 4 + lane16;
#pragma unroll
      for (int u = 0; u < RQ; ++u) {
        rm[u] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_m, boff(vc, rowoff[u]), 0, 0));
        rv[u] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_v, boff(vc, rowoff[u]), 0, 0));
      }
    }
  };
  // out-of-range elements store into this workgroup's 64-float slot behind the dense dlogit
  // tiles (ws_dt holds [n_tiles][B][66] + 64 (grid + 32) floats; the dense layout uses
  // [n_tiles][B][64]), which nothing reads.  One slot per workgroup: a sink shared by all
  // of them would put every workgroup's stores on the same cache lines
  float* const sink = m.ws_dt + (size_t)n_tiles * BM * VB + 64 * (size_t)gfk_bx() + (tid & 63);
  // one 16 x 16 output subtile over the 64-long reduction: ar / bq point at this lane's
  // operand rows, g4 = 4 (lane >> 4); step 4 q + j takes reduction index 16 q + 4 g + j
  // (stored at column (16 q + g4) ^ bx in bq's row: the dtT swizzle)
  auto mm64 = [&](const float* ar, const float* bq, int g4, int bx) {
    f32x4 a[4], b[4];
#pragma unroll
    for (int qq = 0; qq < 4; ++qq) {
      a[qq] = *reinterpret_cast<const f32x4*>(ar + 16 * qq + g4);
      b[qq] = *reinterpret_cast<const f32x4*>(bq + ((16 * qq + g4) ^ bx));
    }
    f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int qq = 0; qq < 4; ++qq) {
      a0 = mfma16x16x4(a[qq][0], b[qq][0], a0);
      a1 = mfma16x16x4(a[qq][1], b[qq][1], a1);
      a0 = mfma16x16x4(a[qq][2], b[qq][2], a0);
      a1 = mfma16x16x4(a[qq][3], b[qq][3], a1);
    }
    return a0 + a1;
  };

  f32x4 dacc[NDT];
#pragma unroll
  for (int j = 0; j < NDT; ++j) dacc[j] = f32x4{0.f, 0.f, 0.f, 0.f};

  f32x4 rm0[RQ], rv0[RQ], rm1[RQ], rv1[RQ];
  issue_bd(slab);
  issue_mv(slab, rm0, rv0);
  // the loop's epilogue issues 3 RU stores after the next tile's loads; the same number of
  // sink stores here gives the loop entry that shape too, so the compiler's wait for the
  // staged registers is vmcnt(3 RU + ...) on both edges (else vmcnt(0) at every tile:
  // the previous tile's stores drained before staging)
  // (addresses the compiler cannot prove equal, so it cannot merge them)
  float* const wsink = sink - (tid & 63);
  constexpr int NST = FUSED ? 3 : 1;           // stores per element in the loop's epilogue
#pragma unroll
  for (int u = 0; u < NST * RQ; ++u) wsink[(tid + 5 * u) & 63] = 0.f;
  auto body = [&](int tile, f32x4 (&rm)[RQ], f32x4 (&rv)[RQ], f32x4 (&nm)[RQ], f32x4 (&nv)[RQ])
      __attribute__((always_inline)) {
    const int c0 = tile * VB;
    asm volatile("" : "+v"(tid));
    __builtin_assume(tid >= 0 && tid < NTH);
    lane = tid & 63;
    wave = uniform(tid >> 6);
    lds_barrier();                             // the previous tile's LDS reads are done
    {
      // (rows past the range / K and columns past V were loaded as 0)
#pragma unroll
      for (int u = 0; u < RQ; ++u)
        *reinterpret_cast<f32x4*>(bt + __mul24((tid >> 4) + RPQ * u, LDP) + 4 * (tid & 15)) = br[u];
#pragma unroll
      for (int j = 0; j < DU; ++j) {           // dense [BM][64] -> dt [b][c] and dtT [c][b]
        const int i = tid + NTH * j, r = i >> 4, c4 = (i & 15) * 4;
        *reinterpret_cast<f32x4*>(dt + __mul24(r, LDP) + c4) = dr[j];
#pragma unroll
        for (int e = 0; e < 4; ++e) dtT[__mul24(c4 + e, LDP) + (r ^ dtt_swz(c4 + e))] = dr[j][e];
      }
    }
    // (KEEP: the beta quads stay in registers for the Adam epilogue -- read back from bt
    // they were the kernel's one conflicting LDS read, 2-way: tools/lds_bank_model.py)
    f32x4 bkeep[KEEP ? RQ : 1];
    if constexpr (KEEP) {
#pragma unroll
      for (int u = 0; u < RQ; ++u) bkeep[u] = br[u];
    }
    // (the staging above consumed the registers) the next tile's beta / dlogit / m / v
    {
      const int tn = min(tile + nslab, n_tiles - 1);    // (last tile: a harmless reload)
      issue_bd(tn);
      issue_mv(tn, nm, nv);
    }
    lds_barrier();

    const int r = lane & 15, g4 = 4 * (lane >> 4);
    // d theta_d[b, k] += sum_c dt[b][c] bt[k][c]
#pragma unroll
    for (int j = 0; j < NDT; ++j) {
      const int t = wave + NW * j;
      if (t >= NDT_T) break;
      const int rt = t / nks, ks = t % nks;
      dacc[j] += mm64(dt + __mul24(rt * 16 + r, LDP), bt + __mul24(ks * 16 + r, LDP), g4, 0);
    }
    // dbeta[k, c] = sum_b thT[k][b] dtT[c][b]
    float gr[MU][4];
#pragma unroll
    for (int u = 0; u < MU; ++u) {
      const int t = wave + NW * u;
      if (t >= NB_T) break;
      const int ks = t >> 2, cst = t & 3;
      const int cr = cst * 16 + r;
      const f32x4 a = mm64(thT + __mul24(ks * 16 + r, LDP), dtT + __mul24(cr, LDP), g4, dtt_swz(cr));
#pragma unroll
      for (int e = 0; e < 4; ++e) gr[u][e] = a[e];
    }
    lds_barrier();                             // every wave is done reading dt / dtT
    float* gt = dtT;                           // the G tile [64 k][64 c], columns XOR 16 (k & 4)
#pragma unroll
    for (int u = 0; u < MU; ++u) {
      const int t = wave + NW * u;
      if (t >= NB_T) break;
      const int ks = t >> 2, cl = (t & 3) * 16 + (lane & 15);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int kl = ks * 16 + (lane >> 4) * 4 + e;
        gt[__mul24(kl, VB) + (cl ^ ((kl & 4) << 2))] = gr[u][e];
      }
    }
    lds_barrier();
    // the G tile, row-wise quads: update (fused) or gradient (the XOR 16 (k & 4) column
    // swizzle keeps a quad's 4 columns together)
    const int kl0 = tid >> 4, c4 = 4 * (tid & 15);
    const int vc = c0 * 4 + lane16;
#pragma unroll
    for (int u = 0; u < RQ; ++u) {
      const int kl = kl0 + RPQ * u;
      const f32x4 gv = *reinterpret_cast<const f32x4*>(gt + __mul24(kl, VB) + (c4 ^ ((kl & 4) << 2)));
      const int vo4 = boff(vc, rowoff[u]);
      if constexpr (FUSED) {
        f32x4 pv;
        if constexpr (KEEP) pv = bkeep[u];
        else pv = *reinterpret_cast<const f32x4*>(bt + __mul24(kl, LDP) + c4);
        f32x4 mo = rm[u], vo = rv[u], np;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float a = mo[e], b2 = vo[e];
          float x = adam_update(pv[e], gv[e], a, b2, ac);
          if (beta_shared && m.fed_scale_on) x *= m.fed_scale;
          mo[e] = a;
          vo[e] = b2;
          np[e] = x;
        }
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(gfk_u32x4, mo), rs_m, vo4, 0, 0);
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(gfk_u32x4, vo), rs_v, vo4, 0, 0);
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(gfk_u32x4, np), rs_b, vo4, 0, 0);
      } else {                                 // the gradient (rs_m is the gradient slot)
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(gfk_u32x4, gv), rs_m, vo4, 0, 0);
      }
    }
  };
#pragma unroll 1
  for (int tile = slab; tile < n_tiles;) {
    body(tile, rm0, rv0, rm1, rv1);
    tile += nslab;
    if (tile >= n_tiles) break;
    body(tile, rm1, rv1, rm0, rv0);
    tile += nslab;
  }
  // this workgroup's d theta_d partial (plain stores; row_bwd sums the slabs in order)
  float* dpart = m.ws_dthetad + (size_t)slab * m.bmax * K;
#pragma unroll
  for (int j = 0; j < NDT; ++j) {
    const int t = wave + NW * j;
    if (t >= NDT_T) break;
    const int rt = t / nks, ks = t % nks;
    const int k = kb + ks * 16 + (lane & 15);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int row = rt * 16 + (lane >> 4) * 4 + e;
      if (row < nb && k < K) dpart[(size_t)row * K + k] = dacc[j][e];
    }
  }
}

// stage_flags bit 2: the strip forward (prodlda_fwd_strip_kernel) -- theta_d + the
// per-wave row partials only
constexpr int FWD_STRIP = 4;
__host__ __device__ inline bool strip_postfold(const GfkModel& m) { return gfk_postfold(m); }
__host__ __device__ inline int strip_pairs(int K) { return (K + 7) / 8; }
// the kernel instance (k pairs in registers) for K
__host__ __device__ inline int strip_np(int K) {
  const int np = strip_pairs(K);
  // (the ring divides NP: 25 pairs (K <= 200) with a ring of 5, 26 = 2 x 13 with 13.
  // K = 200, V = 112k interleaved (profiles/r4/ab_s15): 25 / ring 5 forward 34.9 us, round
  // 0.2625 / 0.2625 ms; 26 / ring 13 (one zero pair) 37.2 us, 0.2647 / 0.2635 ms)
  return np <= 8 ? 8 : np <= 13 ? 13 : np <= 16 ? 16 : np <= 25 ? 25 : np <= 26 ? 26 : 32;
}

// the bf16 strip instance: whole 32-k steps (NP a multiple of 4, ring of 8 pairs)
__host__ __device__ inline int strip_np_bf(int K) { return K <= 64 ? 8 : K <= 128 ? 16 : 32; }

extern "C" size_t gfk_prodlda_fwd_smem(const GfkModel* m) {
  if (m->stage_flags & GFK_LB)                     // (else static LDS only)
    return (m->lb_fused & 1) ? sizeof(float) * lb_fwd_lds_floats(m->K) : 0;
  if (m->stage_flags & FWD_STRIP) {
    const int np = m->mm_bf16 ? strip_np_bf(m->K) : strip_np(m->K);
    // (+ the fused posterior's raw heads [2][B][64] and column statistics [2][128])
    const size_t fp = strip_postfold(*m) ? 2 * (size_t)m->bmax * 64 + 256 : 0;
    return sizeof(float) * ((size_t)m->bmax * (8 * np + 4) + (size_t)(1024 / 64) * m->bmax + fp);
  }
  const size_t KP = round_up(m->K, m->mm_bf16 ? 16 : 4);
  return sizeof(float) * ((size_t)m->bmax * m->kt + KP * LDB_F + 8 * VB);
}

// k ranges of the backward: 4 when the tiles outnumber the workgroups (n_dpart < n_tiles)
// and K has at least 4 k tiles, else 1.  (Also splitting the one-tile-per-workgroup
// headline case, 70 tiles at K=50, was measured: the prologue copy of theta_d's k range
// and the 8-wave dense pass cost more than the quartered MFMA work saved, 0.0652 vs 0.0615
// ms per round.)
__host__ __device__ inline int bwd_kq(const GfkModel& m) {
  return (m.n_dpart < m.n_tiles && round_up(m.K, 16) / 16 >= 4) ? 4 : 1;
}

// the LDS a CU's three 8-wave workgroups may take each (160 KB per CU)
constexpr size_t BWD8_LDS = 160 * 1024 / 3;
static size_t bwd8_smem(const GfkModel* m) {
  const size_t B = m->bmax;
  return sizeof(float) * (B * m->kt + bwd_zb((int)B, bwd_kpq(m->K, 1)) + B * LDD + 2 * B + VB);
}
// whether the 8-wave tile backward (GFK_BWD_BATCH8) has an instance for this model
static bool bwd8_ok(const GfkModel* m) {
  return bwd_kq(*m) == 1 && !m->bwd_pre && m->bmax == 64 && m->K <= 64 && !m->mm_bf16 &&
         bwd8_smem(m) <= BWD8_LDS;
}

static size_t bwd_smem(const GfkModel* m, int kq) {
  const size_t KPQ = bwd_kpq(m->K, kq), B = m->bmax;
  if (kq == 1 && (m->stage_flags & GFK_BWD_BATCH8)) return bwd8_smem(m);
  if (kq == 4 && bwd_pipe(*m)) return sizeof(float) * 4 * 64 * 72;   // thT, bt, dt, dtT
  if (kq == 4 && m->bwd_pre && B <= 64)       // th [B][64] + bt + dt (G aliases dt)
    return sizeof(float) * (B * 64 + KPQ * LDB_B + B * LDD);
  const size_t KTQ = kq == 1 ? (size_t)m->kt : (size_t)kt_stride((int)KPQ);
  return sizeof(float) * (B * KTQ + KPQ * LDB_B + B * VB + B * LDD + 2 * B + VB);
}

// the LDS of the launch shape this model uses (the k-range split when it applies)
extern "C" size_t gfk_prodlda_bwd_smem(const GfkModel* m) {
  if (m->stage_flags & GFK_LB)
    return (m->lb_fused & 2) ? sizeof(float) * lb_bwd_lds_floats(m->K) : 0;
  return bwd_smem(m, bwd_kq(*m));
}

// ---------------------------------------------------------------------------------------
// The instance tables (csrc/gfk_launch.h): a launcher looks its kernel up by the key it
// computes from the model, and gfk_prodlda_set_smem raises the dynamic-LDS limit of the
// same rows.  A new instance is one new row.
// ---------------------------------------------------------------------------------------
// tile forward: {bmax, bf16}
#define FWD_ROW(BM, BF) {{BM, BF}, GFK_PAIR(prodlda_fwd_kernel, BM, BF)}
static const GfkRow kFwdTile[] = {FWD_ROW(16, false), FWD_ROW(32, false), FWD_ROW(64, false), FWD_ROW(128, false),
                                  FWD_ROW(16, true),  FWD_ROW(32, true),  FWD_ROW(64, true),  FWD_ROW(128, true)};
#undef FWD_ROW

// strip forward: {bmax, k pairs (strip_np / strip_np_bf), bf16, postfold}; the postfold
// instances exist for 8 pairs only (gfk_postfold: K <= 64)
#define STRIP_ROW(BM, NP, BF, FP)                                       \
  {{BM, NP, BF, FP}, {prodlda_fwd_strip_kernel<BM, NP, 3, false, BF, FP>, \
                      prodlda_fwd_strip_kernel<BM, NP, 3, true, BF, FP>}}
#define STRIP_ROWS(BM)                                                                             \
  STRIP_ROW(BM, 8, false, false), STRIP_ROW(BM, 13, false, false), STRIP_ROW(BM, 16, false, false), \
  STRIP_ROW(BM, 25, false, false), STRIP_ROW(BM, 26, false, false), STRIP_ROW(BM, 32, false, false), \
  STRIP_ROW(BM, 8, true, false), STRIP_ROW(BM, 16, true, false), STRIP_ROW(BM, 32, true, false),   \
  STRIP_ROW(BM, 8, false, true), STRIP_ROW(BM, 8, true, true)
static const GfkRow kFwdStrip[] = {STRIP_ROWS(16), STRIP_ROWS(32), STRIP_ROWS(64)};
#undef STRIP_ROWS
#undef STRIP_ROW

// backward: {kernel, bmax, 64-topic units (K + 63) / 64, flag}.  kernel: the tile backward
// by its k ranges (1 / 4; flag = bf16), the k-range backward reading the stored logit
// gradient (pre2; flag = bf16), the pipelined one (flag = fused update, bmax 64 only)
// the 8-wave one-range tile backward (BWD_W8; bmax 64, one unit, fp32 only)
enum { BWD_PRE2 = 2, BWD_PIPE = 3, BWD_W8 = 8 };    // (1, 4: the tile backward's KQ)
#define BWD_ROWS_B(BM, U, BF)                                          \
  {{1, BM, U, BF}, GFK_PAIR(prodlda_bwd_kernel, BM, U, 1, BF)},        \
  {{4, BM, U, BF}, GFK_PAIR(prodlda_bwd_kernel, BM, U, 4, BF)}
#define BWD_ROWS_P(BM, U, BF) {{BWD_PRE2, BM, U, BF}, GFK_PAIR(prodlda_bwd_pre2_kernel, BM, U, BF)}
#define BWD_ROWS_F(U, BF)                                                                         \
  BWD_ROWS_B(16, U, BF), BWD_ROWS_B(32, U, BF), BWD_ROWS_B(64, U, BF), BWD_ROWS_B(128, U, BF),    \
  BWD_ROWS_P(16, U, BF), BWD_ROWS_P(32, U, BF), BWD_ROWS_P(64, U, BF),                            \
  {{BWD_PIPE, 64, U, BF}, GFK_PAIR(prodlda_bwd_pipe_kernel, 64, U, BF)}
#define BWD_ROWS(U) BWD_ROWS_F(U, false), BWD_ROWS_F(U, true)
static const GfkRow kBwd[] = {BWD_ROWS(1), BWD_ROWS(2), BWD_ROWS(3), BWD_ROWS(4),
                              {{BWD_W8, 64, 1, false}, GFK_PAIR(prodlda_bwd8_kernel, 64, 1)}};
#undef BWD_ROWS
#undef BWD_ROWS_F
#undef BWD_ROWS_P
#undef BWD_ROWS_B

// the logit gradient ahead of the pre2 / pipelined backward: {bmax}  (static LDS only)
static const GfkRow kDlogit[] = {{{16}, GFK_PAIR(prodlda_dlogit_kernel, 16)},
                                 {{32}, GFK_PAIR(prodlda_dlogit_kernel, 32)},
                                 {{64}, GFK_PAIR(prodlda_dlogit_kernel, 64)}};

// the fused large-batch decoder (one client): {forward 0 / backward 1, k tiles of the instance}
static const GfkRow kLbFused[] = {{{0, 16}, {prodlda_lb_fwd_kernel<16>, nullptr}},
                                  {{0, 32}, {prodlda_lb_fwd_kernel<32>, nullptr}},
                                  {{0, 52}, {prodlda_lb_fwd_kernel<52>, nullptr}},
                                  {{1, 4}, {prodlda_lb_bwd_kernel<4, 16>, nullptr}},
                                  {{1, 8}, {prodlda_lb_bwd_kernel<8, 16>, nullptr}},
                                  {{1, 13}, {prodlda_lb_bwd_kernel<13, 16>, nullptr}}};

// the large-batch column kernels around the GEMMs: {colbn 0 / dlogit 1, bmax}  (static LDS only)
#define LB_ROWS(BM) {{0, BM}, GFK_PAIR(prodlda_lb_colbn_kernel, BM)}, {{1, BM}, GFK_PAIR(prodlda_lb_dlogit_kernel, BM)}
static const GfkRow kLbCol[] = {LB_ROWS(16), LB_ROWS(32), LB_ROWS(64), LB_ROWS(128), LB_ROWS(256), LB_ROWS(512)};
#undef LB_ROWS

static const GfkRow kRowLoss[] = {{{0}, {gfk_prodlda_row_loss<false>, gfk_prodlda_row_loss<true>}}};

// the large-batch kernels (stage_flags GFK_LB): bmax 256 or 512, ws_dt the [bmax][ldb] matrix
static int launch_lb(const GfkModel* m, hipStream_t s, bool fwd) {
  if (m->bmax < 16 || m->bmax > 512 || (m->bmax & (m->bmax - 1)) || m->dec_grid < 1 || m->ldb < m->V ||
      m->n_batch > 1)
    return -1;
  if ((int64_t)(m->K + 16) * m->ldb * 4 >= 0x7FFF0000LL) return -1;     // 32-bit buffer offsets
  if (fwd && (m->lb_fused & 1)) {
    if (m->bmax != 256 || m->K > 208 || m->kind != GFK_PRODLDA) return -1;
    const size_t sm = sizeof(float) * lb_fwd_lds_floats(m->K);
    return gfk_launch(gfk_find(kLbFused, 0, m->K <= 64 ? 16 : m->K <= 128 ? 32 : 52), m,
                      dim3(m->dec_grid), dim3(LBF_NT), sm, s);
  }
  if (!fwd && (m->lb_fused & 2)) {
    if (m->bmax != 256 || m->K > 208 || m->update_mode != 0 || m->n_dpart != m->dec_grid) return -1;
    const size_t sm = sizeof(float) * lb_bwd_lds_floats(m->K);
    return gfk_launch(gfk_find(kLbFused, 1, m->K <= 64 ? 4 : m->K <= 128 ? 8 : 13), m,
                      dim3(m->dec_grid), dim3(1024), sm, s);
  }
  if (!m->ws_dt) return -1;
  // (bmax below 256: K > 256 at the batch's own size)
  return gfk_launch(gfk_find(kLbCol, fwd ? 0 : 1, m->bmax), m, dim3(m->dec_grid), dim3(LB_THREADS), 0, s);
}

extern "C" int gfk_launch_prodlda_fwd(const GfkModel* m, hipStream_t s) {
  if (m->stage_flags & GFK_LB) return launch_lb(m, s, true);
  const size_t sm = gfk_prodlda_fwd_smem(m);
  dim3 g(m->dec_grid), blk(DEC_THREADS);
  if (m->stage_flags & FWD_STRIP) {
    // fp32, B <= 64, K <= 256; the partial slots need 4 * grid <= 4 * n_tiles
    if (m->bmax > 64 || m->K > 256 || m->dec_grid > m->n_tiles ||
        (int64_t)m->K * m->ldb >= (1LL << 29)) return -1;
    const bool bf = m->mm_bf16;
    const int np = bf ? strip_np_bf(m->K) : strip_np(m->K);
    return gfk_launch(gfk_find(kFwdStrip, m->bmax, np, bf, strip_postfold(*m)), m, g,
                      dim3(strip_threads(3, np)), sm, s);
  }
  return gfk_launch(gfk_find(kFwdTile, m->bmax, (bool)m->mm_bf16), m, g, blk, sm, s);
}

extern "C" int gfk_launch_prodlda_bwd(const GfkModel* m, hipStream_t s) {
  if (m->stage_flags & GFK_LB) return launch_lb(m, s, false);
  if (m->bmax != 16 && m->bmax != 32 && m->bmax != 64 && m->bmax != 128) return -1;
  if ((int64_t)m->K * m->ldb * 4 >= 0x7FFF0000LL) return -1;   // 32-bit buffer offsets
  const int maxu = (m->K + 63) / 64;
  const int kq = bwd_kq(*m);
  const int slabs = m->n_dpart < m->n_tiles ? m->n_dpart : m->n_tiles;
  const size_t sm = bwd_smem(m, kq);
  const dim3 g(kq == 4 ? 4 * slabs : slabs), blk(kq == 1 ? DEC_THREADS : 512);
  const bool bf = m->mm_bf16;
  if (m->stage_flags & GFK_BWD_BATCH8) {             // (no instance: an error, never the 16-wave shape)
    if (!bwd8_ok(m)) return -1;
    return gfk_launch(gfk_find(kBwd, BWD_W8, m->bmax, maxu, false), m, g, dim3(512), sm, s);
  }
  if (kq == 4 && m->bwd_pre && m->bmax <= 64) {      // (static LDS: B <= 64)
    const int e = gfk_launch(gfk_find(kDlogit, m->bmax), m, dim3(m->n_tiles), dim3(256), 0, s);
    if (e) return e;
    // (the pipelined backward also serves mm_bf16: its GEMMs keep fp32 operands -- the
    // kernel is bound by its beta / Adam-state HBM traffic, not by the matrix cores)
    if (bwd_pipe(*m)) return gfk_launch(gfk_find(kBwd, BWD_PIPE, 64, maxu, m->update_mode == 1), m, g, blk, sm, s);
    return gfk_launch(gfk_find(kBwd, BWD_PRE2, m->bmax, maxu, bf), m, g, blk, sm, s);
  }
  return gfk_launch(gfk_find(kBwd, kq, m->bmax, maxu, bf), m, g, blk, sm, s);
}

extern "C" int gfk_launch_prodlda_row_loss(const GfkModel* m, hipStream_t s) {
  return gfk_launch(gfk_find(kRowLoss, 0), m, dim3(m->bmax), dim3(64), 0, s);
}

// (the dynamic-LDS tables; kDlogit, kLbCol and kRowLoss are launched with none)
extern "C" int gfk_prodlda_set_smem(size_t bytes) {
  static size_t cur = 0;
  if (!gfk_lds_raised(cur, bytes)) return 0;
  int e = gfk_raise_lds(kFwdTile, bytes);
  if (!e) e = gfk_raise_lds(kFwdStrip, bytes);
  if (!e) e = gfk_raise_lds(kBwd, bytes);
  if (!e) e = gfk_raise_lds(kLbFused, bytes);
  return e;
}
