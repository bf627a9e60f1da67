// Bhattacharyya similarity scores in float64 on the matrix cores:
//
//   DSS = sum_{d,e} | sqrt(A_d) . sqrt(A_e) - sqrt(B_d) . sqrt(B_e) | / n_docs      gfk_dss
//   BC[i][j] = sqrt(X_i) . sqrt(Y_j),   TSS = sum_j max_i BC[i][j]                   gfk_bc
//
// (eval/metrics.py dss / tss: A = ground-truth thetas [D, Ka], B = the model's [D, Kb];
// X = learned topics [M, L], Y = ground-truth topics [N, L].)  All arithmetic is float64
// whatever the inputs' type (fp32 inputs are widened, which is exact), there are no atomics,
// and every sum runs in an order that is a function of the shape alone, so the results do not
// depend on the grid bit for bit.  DSS never holds more than one 64 x 64 tile of either
// D x D similarity matrix.
//
// ss_tile: one 64 x 64 tile of sqrt(X_I) sqrt(Y_J)^T over a range of the reduction axis, by
// 4 waves as 2 x 2 blocks of 32 x 32, each four v_mfma_f64_16x16x4_f64 accumulators.  The
// reduction axis is staged through LDS 16 columns at a time: 64 rows of each operand are
// converted to f64 and square-rooted (the correctly rounded sqrt: the build's fp32 flags do
// not touch the f64 one) on the way in, rows past the end and columns past the range as
// zeros, which contribute exactly 0, so nothing downstream is masked.  A chunk's global loads
// are issued one chunk ahead, into registers, under the previous chunk's MFMAs -- across the
// two products of a DSS item and across items as well.  LDS row stride 18 doubles: the 16
// rows x 2 k a half-wave's ds_read_b64 covers fall on 32 distinct 8-byte bank pairs
// (18 row + k mod 32; tools/lds_bank_model.py simscore_accesses).  A lane's operand is
// X[i = lane & 15][k = lane >> 4] (and Y likewise, as B[k][j]); its four results of a 16 x 16
// block are col = lane & 15, row = (lane >> 4) + 4 reg.
//
// gfk_dss: a work item is a pair of row tiles I <= J in row-major order of the upper
// triangle; persistent workgroups stride over the items.  An item takes both products of its
// (I, J) with ss_tile, sums |Sa - Sb| over the lane's registers, the wave's lanes (xor
// butterfly) and the four waves (LDS, in wave order), doubles it off the diagonal (exact)
// and stores partial[item].  gfk_dss_sum_k, one workgroup, adds the partials: thread t takes
// items t, t + 1024, ... in order, then a fixed tree -- a function of the item count alone --
// and divides by n_docs.
//
// gfk_bc: a work item is (output tile, range of L); the number of ranges is a function of L
// alone (ss_ranges).  Items store their tile of part[range][M][N]; gfk_bc_merge_k adds the
// ranges in range order into BC, and gfk_bc_tss_k, one workgroup, takes each column's
// maximum and adds the columns in index order.
#include "gfk_common.h"

extern "C" {
typedef struct GfkDss {
  const void *a, *b;        // A [D, Ka] ground truth, B [D, Kb]: row-major fp32 or fp64
  double* part;             // workspace: one partial per tile pair
  double* out;              // the scalar
  int64_t lda, ldb;         // row strides, in elements
  int64_t n_docs;           // the divisor
  int64_t part_len;         // capacity of part, in doubles
  int32_t D, Ka, Kb;
  int32_t a_f64, b_f64;     // 1: fp64 input, 0: fp32
  int32_t max_grid;         // > 0: at most this many workgroups (tests); 0: the default
} GfkDss;

typedef struct GfkBc {
  const void *x, *y;        // X [M, L], Y [N, L]: row-major fp32 or fp64
  double* part;             // workspace [ranges, M, N]
  double* bc;               // BC [M, N]
  double* tss;              // the scalar sum_j max_i BC[i][j], or null
  int64_t ldx, ldy;         // row strides, in elements
  int64_t part_len;         // capacity of part, in doubles
  int32_t M, N, L;
  int32_t x_f64, y_f64;
  int32_t max_grid;
} GfkBc;
}

namespace {

constexpr int SS_T = 64;            // rows per tile
constexpr int SS_KC = 16;           // reduction columns per staged chunk
constexpr int SS_LD = SS_KC + 2;    // LDS row stride (doubles)
constexpr int SS_THREADS = 256;
constexpr int SS_MAX_K = 512;       // K of gfk_dss, M and N of gfk_bc
constexpr int SS_GRID = 1024;       // default persistent grid (4 workgroups per CU)
constexpr int SS_SUM_THREADS = 1024;
constexpr int SS_RANGE = 1024;      // reduction columns a range aims for
constexpr int SS_MAX_RANGES = 32;

typedef double f64x4 __attribute__((ext_vector_type(4)));

__host__ __device__ inline int ss_ranges(int L) {
  const int r = (L + SS_RANGE - 1) / SS_RANGE;
  return r < 1 ? 1 : (r > SS_MAX_RANGES ? SS_MAX_RANGES : r);
}
// columns per range: whole chunks
__host__ __device__ inline int ss_range_len(int L) {
  const int chunks = (L + SS_KC - 1) / SS_KC, nr = ss_ranges(L);
  return (chunks + nr - 1) / nr * SS_KC;
}

// The operands of one tile product: rows [i0, i0 + 64) of x against rows [j0, j0 + 64) of y
// over columns [c0, c1).  same: y's rows are x's (a diagonal tile of X X^T), staged once.
// c0 >= c1: nothing to do.
struct SsOp {
  const void *x, *y;
  int64_t ldx, ldy;
  int x64, y64, nx, ny, i0, j0, c0, c1;
  bool same;
};

constexpr int SS_PER = SS_T * SS_KC / SS_THREADS;   // elements of a chunk per thread and operand

// a thread's share of the next chunk, as loaded (before the square root)
struct SsRaw {
  double x[SS_PER], y[SS_PER];
};

// rows [r0, r0 + 64) x columns [c0, c0 + 16) of src as f64; zero past n_rows / c1
__device__ inline void ss_load1(double (&v)[SS_PER], const void* src, int is64, int64_t ld, int r0,
                                int n_rows, int c0, int c1) {
#pragma unroll
  for (int k = 0; k < SS_PER; ++k) {
    const int idx = threadIdx.x + k * SS_THREADS;
    const int r = idx / SS_KC, c = idx % SS_KC;
    v[k] = 0.0;
    if (r0 + r < n_rows && c0 + c < c1) {
      const size_t at = (size_t)(r0 + r) * (size_t)ld + (size_t)(c0 + c);
      v[k] = is64 ? ((const double*)src)[at] : (double)((const float*)src)[at];
    }
  }
}

__device__ inline void ss_load(SsRaw& raw, const SsOp& o, int cb) {
  ss_load1(raw.x, o.x, o.x64, o.ldx, o.i0, o.nx, cb, o.c1);
  if (!o.same) ss_load1(raw.y, o.y, o.y64, o.ldy, o.j0, o.ny, cb, o.c1);
}

// the square roots of a loaded chunk into its LDS tile
__device__ inline void ss_store1(double* dst, const double (&v)[SS_PER]) {
#pragma unroll
  for (int k = 0; k < SS_PER; ++k) {
    const int idx = threadIdx.x + k * SS_THREADS;
    dst[idx / SS_KC * SS_LD + idx % SS_KC] = sqrt(v[k]);
  }
}

// acc[m][n] += the 16 x 16 blocks (2 wr + m, 2 wc + n) of sqrt(X[i0 .. i0 + 64)) sqrt(Y[j0 ..
// j0 + 64))^T over o's columns.  On entry raw holds o's first chunk; while a chunk is
// multiplied the next one -- o's, or after o's last the first of `next` -- is loaded into raw,
// so the global loads run under the MFMAs and raw is ready for ss_tile(next).  Ends on a
// barrier: LDS may be reused at once.
__device__ inline void ss_tile(f64x4 (&acc)[2][2], double* sx, double* sy, SsRaw& raw,
                               const SsOp& o, const SsOp& next) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int lr = lane & 15, kq = lane >> 4;
  const double* ty = o.same ? sx : sy;
  if (o.c0 >= o.c1 && next.c0 < next.c1) ss_load(raw, next, next.c0);
  for (int cb = o.c0; cb < o.c1; cb += SS_KC) {
    ss_store1(sx, raw.x);
    if (!o.same) ss_store1(sy, raw.y);
    __syncthreads();
    if (cb + SS_KC < o.c1) ss_load(raw, o, cb + SS_KC);
    else if (next.c0 < next.c1) ss_load(raw, next, next.c0);
    // whole k-steps of 4 that hold a column of the range (the rest of the chunk is zeros)
    const int kend = o.c1 - cb < SS_KC ? (o.c1 - cb + 3) & ~3 : SS_KC;
#pragma unroll
    for (int k = 0; k < SS_KC; k += 4) {
      if (k >= kend) break;
      double a[2], b[2];
#pragma unroll
      for (int m = 0; m < 2; ++m) a[m] = sx[(32 * wr + 16 * m + lr) * SS_LD + k + kq];
#pragma unroll
      for (int n = 0; n < 2; ++n) b[n] = ty[(32 * wc + 16 * n + lr) * SS_LD + k + kq];
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n)
          acc[m][n] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[m], b[n], acc[m][n], 0, 0, 0);
    }
    __syncthreads();
  }
}

__device__ inline void ss_zero(f64x4 (&acc)[2][2]) {
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n) acc[m][n] = f64x4{0.0, 0.0, 0.0, 0.0};
}

// first item of tile row I in the row-major upper triangle of nt x nt tiles
__device__ inline long long ss_row_start(long long I, long long nt) { return I * nt - I * (I - 1) / 2; }

// tile pair (I, J) of an item: I from the triangle's closed form, corrected by the exact
// integer row starts
__device__ inline void ss_pair(int item, int nt, int& I, int& J) {
  const double h = nt + 0.5;
  I = (int)(h - sqrt(h * h - 2.0 * (double)item));
  I = I < 0 ? 0 : (I > nt - 1 ? nt - 1 : I);
  while (I + 1 < nt && ss_row_start(I + 1, nt) <= item) ++I;
  while (I > 0 && ss_row_start(I, nt) > item) --I;
  J = I + (int)(item - ss_row_start(I, nt));
}

// rows I against rows J of one [D, K] input
__device__ inline SsOp ss_dss_op(const void* src, int is64, int64_t ld, int D, int K, int I, int J) {
  return SsOp{src, src, ld, ld, is64, is64, D, D, I * SS_T, J * SS_T, 0, K, I == J};
}

__global__ void __launch_bounds__(SS_THREADS) gfk_dss_k(GfkDss p, int nt, int n_items) {
  __shared__ double sx[SS_T * SS_LD], sy[SS_T * SS_LD];
  __shared__ double wsum[SS_THREADS / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int item = blockIdx.x, I, J;
  if (item >= n_items) return;
  ss_pair(item, nt, I, J);
  SsOp oa = ss_dss_op(p.a, p.a_f64, p.lda, p.D, p.Ka, I, J);
  SsRaw raw;
  ss_load(raw, oa, 0);
  for (;;) {
    const SsOp ob = ss_dss_op(p.b, p.b_f64, p.ldb, p.D, p.Kb, I, J);
    const int nitem = item + gridDim.x;
    int NI = 0, NJ = 0;
    SsOp na = oa;
    na.c1 = 0;                               // (no next item: nothing to load)
    if (nitem < n_items) {
      ss_pair(nitem, nt, NI, NJ);
      na = ss_dss_op(p.a, p.a_f64, p.lda, p.D, p.Ka, NI, NJ);
    }
    f64x4 sa[2][2], sb[2][2];
    ss_zero(sa);
    ss_zero(sb);
    ss_tile(sa, sx, sy, raw, oa, ob);
    ss_tile(sb, sx, sy, raw, ob, na);
    double s = 0.0;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int r = 0; r < 4; ++r) s += fabs(sa[m][n][r] - sb[m][n][r]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) wsum[wave] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
      const double t = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
      p.part[item] = I == J ? t : 2.0 * t;
    }
    __syncthreads();                         // wsum is rewritten by the next item
    if (nitem >= n_items) break;
    item = nitem;
    I = NI;
    J = NJ;
    oa = na;
  }
}

__global__ void __launch_bounds__(SS_SUM_THREADS) gfk_dss_sum_k(GfkDss p, int n_items) {
  __shared__ double red[SS_SUM_THREADS];
  const int t = threadIdx.x;
  double s = 0.0;
  for (int i = t; i < n_items; i += SS_SUM_THREADS) s += p.part[i];
  red[t] = s;
  __syncthreads();
  for (int o = SS_SUM_THREADS / 2; o > 0; o >>= 1) {
    if (t < o) red[t] += red[t + o];
    __syncthreads();
  }
  if (t == 0) *p.out = red[0] / (double)p.n_docs;
}

// tile and range of an item: ranges vary fastest
__device__ inline SsOp ss_bc_op(const GfkBc& p, int ntn, int item, int& rg) {
  const int nr = ss_ranges(p.L), rlen = ss_range_len(p.L);
  rg = item % nr;
  const int tile = item / nr, c0 = rg * rlen;
  const int c1 = c0 + rlen < p.L ? c0 + rlen : p.L;     // (c0 >= L: an empty range, zeros)
  return SsOp{p.x, p.y, p.ldx, p.ldy, p.x_f64, p.y_f64, p.M, p.N, tile / ntn * SS_T,
              tile % ntn * SS_T, c0, c1, false};
}

__global__ void __launch_bounds__(SS_THREADS) gfk_bc_k(GfkBc p, int ntn, int n_items) {
  __shared__ double sx[SS_T * SS_LD], sy[SS_T * SS_LD];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  int item = blockIdx.x, rg, nrg = 0;
  if (item >= n_items) return;
  SsOp o = ss_bc_op(p, ntn, item, rg);
  SsRaw raw;
  if (o.c0 < o.c1) ss_load(raw, o, o.c0);
  for (;;) {
    const int nitem = item + gridDim.x;
    SsOp next = o;
    next.c1 = next.c0;                       // (no next item: nothing to load)
    if (nitem < n_items) next = ss_bc_op(p, ntn, nitem, nrg);
    f64x4 acc[2][2];
    ss_zero(acc);
    ss_tile(acc, sx, sy, raw, o, next);
    double* out = p.part + (size_t)rg * p.M * p.N;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = o.i0 + 32 * wr + 16 * m + (lane >> 4) + 4 * r;
          const int j = o.j0 + 32 * wc + 16 * n + (lane & 15);
          if (i < p.M && j < p.N) out[(size_t)i * p.N + j] = acc[m][n][r];
        }
    if (nitem >= n_items) break;
    item = nitem;
    rg = nrg;
    o = next;
  }
}

__global__ void __launch_bounds__(SS_THREADS) gfk_bc_merge_k(GfkBc p) {
  const int nr = ss_ranges(p.L);
  const size_t mn = (size_t)p.M * p.N;
  for (size_t e = (size_t)blockIdx.x * SS_THREADS + threadIdx.x; e < mn;
       e += (size_t)gridDim.x * SS_THREADS) {
    double s = p.part[e];
    for (int r = 1; r < nr; ++r) s += p.part[(size_t)r * mn + e];
    p.bc[e] = s;
  }
}

__global__ void __launch_bounds__(SS_THREADS) gfk_bc_tss_k(GfkBc p) {
  __shared__ double cmax[SS_MAX_K];
  for (int j = threadIdx.x; j < p.N; j += SS_THREADS) {
    double m = p.bc[j];
    for (int i = 1; i < p.M; ++i) {
      const double v = p.bc[(size_t)i * p.N + j];
      m = v > m ? v : m;
    }
    cmax[j] = m;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int j = 0; j < p.N; ++j) s += cmax[j];
    *p.tss = s;
  }
}

}  // namespace

extern "C" size_t gfk_dss_struct_size() { return sizeof(GfkDss); }
extern "C" size_t gfk_bc_struct_size() { return sizeof(GfkBc); }

// the largest K of gfk_dss and M, N of gfk_bc
extern "C" int gfk_sim_max_rows() { return SS_MAX_K; }

// tile pairs of gfk_dss = doubles of its workspace; -1 when they do not fit an int
extern "C" int64_t gfk_dss_items(int64_t D) {
  if (D < 0) return -1;
  const int64_t nt = (D + SS_T - 1) / SS_T;
  const int64_t items = nt * (nt + 1) / 2;
  return items < ((int64_t)1 << 31) ? items : -1;
}

// ranges of the reduction axis of gfk_bc (its workspace is ranges * M * N doubles)
extern "C" int gfk_bc_ranges(int L) { return ss_ranges(L); }

// Host checks mirror the kernels' assumptions: 1 <= Ka, Kb <= 512, row strides that hold a
// row, D in an int with its tile pairs in an int, a workspace of one double per pair.
// Nothing is launched when a check fails.  D = 0 stores 0.
extern "C" int gfk_dss(const GfkDss* p, hipStream_t s) {
  if (!p) return -7;
  if (p->Ka < 1 || p->Ka > SS_MAX_K || p->Kb < 1 || p->Kb > SS_MAX_K || p->max_grid < 0) return -5;
  if (p->D < 0 || p->n_docs < 1 || p->lda < p->Ka || p->ldb < p->Kb) return -6;
  const int64_t items = gfk_dss_items(p->D);
  if (items < 0) return -6;
  if (!p->out) return -7;
  if (p->D == 0) return (int)hipMemsetAsync(p->out, 0, sizeof(double), s);
  if (!p->a || !p->b || !p->part) return -7;
  if (p->part_len < items) return -9;
  const int nt = (p->D + SS_T - 1) / SS_T;
  int grid = items < SS_GRID ? (int)items : SS_GRID;
  if (p->max_grid > 0 && grid > p->max_grid) grid = p->max_grid;
  hipLaunchKernelGGL(gfk_dss_k, dim3(grid), dim3(SS_THREADS), 0, s, *p, nt, (int)items);
  int rc = (int)hipGetLastError();
  if (rc) return rc;
  hipLaunchKernelGGL(gfk_dss_sum_k, dim3(1), dim3(SS_SUM_THREADS), 0, s, *p, (int)items);
  return (int)hipGetLastError();
}

// 1 <= M, N <= 512, L >= 1, row strides that hold a row, a workspace of gfk_bc_ranges(L) * M * N
// doubles.  tss may be null (the matrix alone).
extern "C" int gfk_bc(const GfkBc* p, hipStream_t s) {
  if (!p) return -7;
  if (p->M < 1 || p->M > SS_MAX_K || p->N < 1 || p->N > SS_MAX_K || p->max_grid < 0) return -5;
  if (p->L < 1 || p->ldx < p->L || p->ldy < p->L) return -6;
  if (!p->x || !p->y || !p->part || !p->bc) return -7;
  const int nr = ss_ranges(p->L);
  if (p->part_len < (int64_t)nr * p->M * p->N) return -9;
  const int ntm = (p->M + SS_T - 1) / SS_T, ntn = (p->N + SS_T - 1) / SS_T;
  const int items = ntm * ntn * nr;          // <= 8 * 8 * 32
  int grid = items;
  if (p->max_grid > 0 && grid > p->max_grid) grid = p->max_grid;
  hipLaunchKernelGGL(gfk_bc_k, dim3(grid), dim3(SS_THREADS), 0, s, *p, ntn, items);
  int rc = (int)hipGetLastError();
  if (rc) return rc;
  int mgrid = (p->M * p->N + SS_THREADS - 1) / SS_THREADS;
  hipLaunchKernelGGL(gfk_bc_merge_k, dim3(mgrid), dim3(SS_THREADS), 0, s, *p);
  rc = (int)hipGetLastError();
  if (rc || !p->tss) return rc;
  hipLaunchKernelGGL(gfk_bc_tss_k, dim3(1), dim3(SS_THREADS), 0, s, *p);
  return (int)hipGetLastError();
}
