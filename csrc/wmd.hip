// Word mover's distance between topic word lists: batched exact optimal transport in float64.
//
//   c_ij = || a_i - b_j ||_2                                                        gfk_wmd_dist
//   WMD(A, B) = min sum f_ij c_ij,  rows of f sum to 1/n, columns to 1/m, f >= 0   gfk_wmd_solve
//
// (eval/metrics.py word_movers_distance / mean_min_wmd: A, B = the top words of two topics, the
// vectors = word embeddings.)  No atomics; every sum runs in an order that is a function of the
// shape alone, so no result depends on the grid, on a problem's place in its batch or on its
// neighbours, bit for bit.
//
// gfk_wmd_dist: D[Ua, Ub] from two sets of gathered word vectors (fp32 or fp64, widened, which is
// exact), 64 x 64 tiles by 256 threads of 4 x 4 outputs each, the vectors staged through LDS 16
// dimensions at a time.  The difference form sqrt(sum_d (a_d - b_d)^2), d in index order, no
// contraction: identical vectors cost exactly 0.0.  Rows past the end and dimensions past dim
// are staged as zeros on both sides, which add exactly 0.  The float64 sqrt is the correctly
// rounded one (the build's fp32 flags do not touch it).
//
// gfk_wmd_solve: problem (ia, ib) = list ia of row indices against list ib of column indices
// into one D; the lists come from device offset tables.  In integer units (g = gcd(n, m)) every
// source supplies m / g, every sink takes n / g, T = n m / g units flow.  Successive shortest
// paths with node potentials p, q (float64, from 0), reduced cost rc_ij = max(c_ij + p_i - q_j,
// 0), integer flow x.  For each source r in index order, at most T times while it has supply:
//   1. Dijkstra from r over the n + m nodes, at most n + m visits: the unvisited node of least
//      distance (ties: a source before a sink, then the lower index); a source i relaxes every
//      unvisited sink with dS_i + rc_ij; a sink with residual demand ends the search (the
//      target, at distance delta); a saturated sink j relaxes every unvisited source k that has
//      x_kj > 0 with dT_j - rc_kj;
//   2. p_i += min(dS_i, delta), q_j += min(dT_j, delta) (unreached nodes hold inf);
//   3. the bottleneck of the supply, the target's demand and the path's backward arcs is pushed
//      along the predecessor chain.
// The value is sum_i (sum_j x_ij c_ij) / T: row sums in j order, added in i order, one division.
// Every loop has a static bound; a search without a target or a bound that is hit leaves the
// loops with status != 0 (neither happens on valid input).
//
// One wavefront per problem, no barriers.  Lane l owns sources and sinks l, l + 64, ...: their
// distances dS, dT and visited bits live in its registers (only the owner touches
// them; the popped node's distance comes out of the argmin itself).  The argmin is a wave-wide
// lexicographic (distance, node id) minimum -- DPP inside the 16-lane rows, two cross-lane
// exchanges above -- a total order, so it does not depend on the lane layout.  What a node
// visit or the augmentation reads of ANOTHER lane's node sits in the wave's slice of LDS:
// p, q (float64), the D indices (int32), the predecessors and the sinks' residual demands (uint16).  The flow is a
// uint16 [m][n] (sink-major: a sink visit reads one row of it, the augmentation single entries)
// in a global workspace slot per resident wave, zeroed by the wave before every problem.
// Workgroups of 4 waves are persistent over the problem indices.  Two capacity instances, <= 128
// and <= 512 words per list (15 KB and 60 KB of LDS per workgroup, NK = 2 and 8 owned nodes per
// lane and side), chosen by the batch's longest list.
#include "gfk_common.h"

extern "C" {
typedef struct GfkWmdDist {
  const void *a, *b;        // vectors [Ua, dim], [Ub, dim]: row-major fp32 or fp64
  double* out;              // D [Ua, Ub]
  int64_t lda, ldb, ldo;    // row strides, in elements
  int32_t Ua, Ub, dim;
  int32_t a_f64, b_f64;     // 1: fp64 input, 0: fp32
  int32_t max_grid;         // > 0: at most this many workgroups (tests); 0: the default
} GfkWmdDist;

typedef struct GfkWmd {
  const double* dist;       // D [Ua, Ub]
  const int32_t *a_off, *a_idx;   // [La + 1] offsets into a_idx: rows of D of every list
  const int32_t *b_off, *b_idx;   // [Lb + 1] offsets into b_idx: columns of D
  uint16_t* flow;           // workspace: slot_len entries per wave of the grid
  double* val;              // [La, Lb]
  int32_t* status;          // [La, Lb]
  int64_t ldd;              // row stride of D, in elements
  int64_t flow_len;         // capacity of flow, in entries
  int32_t Ua, Ub, La, Lb;
  int32_t max_a, max_b;     // the longest list of either side
  int32_t cap;              // 0: by the longest list; 128 / 512: that instance (tests)
  int32_t max_grid;
} GfkWmd;
}

#pragma clang fp contract(off)

namespace {

constexpr int WD_T = 64;            // rows / columns per tile of gfk_wmd_dist
constexpr int WD_DC = 16;           // dimensions per staged chunk
constexpr int WD_LD = WD_DC + 1;    // LDS row stride (doubles): 16 consecutive rows, 16 bank pairs
constexpr int WD_THREADS = 256;
constexpr int WD_GRID = 1024;

constexpr int WM_MAX = 512;         // words per list
constexpr int WM_SMALL = 128;       // ... of the small instance
constexpr int WM_WAVES = 4;         // waves (problems in flight) per workgroup
constexpr int WM_THREADS = WM_WAVES * 64;
constexpr int WM_GRID_SMALL = 1024; // default persistent grids: 4 / 2 workgroups per CU (the
constexpr int WM_GRID_LARGE = 512;  // large instance's 60 KB of LDS allow two)
constexpr int WM_NONE = 0x7fffffff; // node id of "no unvisited node"

// rows [r0, r0 + 64) x dimensions [d0, d0 + 16) of src as f64 into dst[64][WD_LD]; zeros past
// n_rows / dim
__device__ inline void wd_stage(double* dst, const void* src, int is64, int64_t ld, int r0,
                                int n_rows, int d0, int dim) {
#pragma unroll
  for (int k = 0; k < WD_T * WD_DC / WD_THREADS; ++k) {
    const int idx = threadIdx.x + k * WD_THREADS;
    const int r = idx / WD_DC, c = idx % WD_DC;
    double v = 0.0;
    if (r0 + r < n_rows && d0 + c < dim) {
      const size_t at = (size_t)(r0 + r) * (size_t)ld + (size_t)(d0 + c);
      v = is64 ? ((const double*)src)[at] : (double)((const float*)src)[at];
    }
    dst[r * WD_LD + c] = v;
  }
}

__global__ void __launch_bounds__(WD_THREADS) gfk_wmd_dist_k(GfkWmdDist p, int ntb, int n_tiles) {
  __shared__ double sa[WD_T * WD_LD], sb[WD_T * WD_LD];
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int i0 = tile / ntb * WD_T, j0 = tile % ntb * WD_T;
    double acc[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[r][c] = 0.0;
    for (int d0 = 0; d0 < p.dim; d0 += WD_DC) {
      wd_stage(sa, p.a, p.a_f64, p.lda, i0, p.Ua, d0, p.dim);
      wd_stage(sb, p.b, p.b_f64, p.ldb, j0, p.Ub, d0, p.dim);
      __syncthreads();
#pragma unroll
      for (int d = 0; d < WD_DC; ++d) {
        double a[4], b[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) a[r] = sa[(ty + 16 * r) * WD_LD + d];
#pragma unroll
        for (int c = 0; c < 4; ++c) b[c] = sb[(tx + 16 * c) * WD_LD + d];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const double df = a[r] - b[c];
            acc[r][c] = acc[r][c] + df * df;
          }
      }
      __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int i = i0 + ty + 16 * r, j = j0 + tx + 16 * c;
        if (i < p.Ua && j < p.Ub) p.out[(size_t)i * (size_t)p.ldo + j] = sqrt(acc[r][c]);
      }
  }
}

// ---- the solver --------------------------------------------------------------------------

template <int CAP>
struct WmLds {
  double p[CAP], q[CAP];
  uint16_t pS[CAP], pT[CAP];   // predecessor sink of a source, predecessor source of a sink
  uint16_t t[CAP];             // residual demand of a sink
  int32_t ri[CAP], cj[CAP];    // row of D of a source, column of a sink
};

template <int CTRL>
__device__ __forceinline__ int wm_dpp(int v) {
  return __builtin_amdgcn_update_dpp(v, v, CTRL, 0xF, 0xF, false);
}

// (d, id) <- the lexicographically smaller of itself and (od, oid)
__device__ __forceinline__ void wm_take(double& d, int& id, double od, int oid) {
  const bool less = od < d || (od == d && oid < id);
  d = less ? od : d;
  id = less ? oid : id;
}

template <int CTRL>
__device__ __forceinline__ void wm_min_dpp(double& d, int& id) {
  const int lo = wm_dpp<CTRL>(__double2loint(d)), hi = wm_dpp<CTRL>(__double2hiint(d));
  const int oid = wm_dpp<CTRL>(id);
  wm_take(d, id, __hiloint2double(hi, lo), oid);
}

// the wave's least (distance, node id) in every lane, the id wave-uniform for the compiler as
// well (the distance stays in vector registers: the scalar file is the scarce one): quad_perm
// xor 1 / xor 2, row_half_mirror, row_mirror cover a 16-lane row, xor 16 / 32 the rest
__device__ __forceinline__ void wm_argmin(double& d, int& id) {
  wm_min_dpp<0xB1>(d, id);
  wm_min_dpp<0x4E>(d, id);
  wm_min_dpp<0x141>(d, id);
  wm_min_dpp<0x140>(d, id);
#pragma unroll
  for (int o = 16; o <= 32; o <<= 1) {
    const double od = __shfl_xor(d, o, 64);
    const int oid = __shfl_xor(id, o, 64);
    wm_take(d, id, od, oid);
  }
  id = __builtin_amdgcn_readfirstlane(id);
}

// orders the wave's own global stores before its later loads of the same addresses by other
// lanes (flow entries; one L1, so completion in order is all that is needed)
__device__ __forceinline__ void wm_flow_fence() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
}

// a value every lane read from one address, as a scalar for the compiler
__device__ __forceinline__ int wm_u(int v) { return __builtin_amdgcn_readfirstlane(v); }

__host__ __device__ inline int wm_gcd(int a, int b) {
  for (int it = 0; it < 64 && b; ++it) {      // (Euclid on values <= 512: < 16 steps)
    const int r = a % b;
    a = b;
    b = r;
  }
  return a;
}

// entries of a wave's flow slot: the batch's largest n m, in whole 16-byte stores
__host__ __device__ inline int wm_slot_len(int max_a, int max_b) { return (max_a * max_b + 7) & ~7; }

template <int CAP>
__global__ void __launch_bounds__(WM_THREADS) gfk_wmd_solve_k(GfkWmd a, int n_prob) {
  constexpr int NK = CAP / 64;
  __shared__ WmLds<CAP> lds[WM_WAVES];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  WmLds<CAP>& L = lds[wave];
  const int slot = blockIdx.x * WM_WAVES + wave, n_slots = gridDim.x * WM_WAVES;
  const int slot_len = wm_slot_len(a.max_a, a.max_b);
  // (the slot's base as a vector-register pair: the scalar file is the scarce one here)
  uint16_t* x = a.flow + (size_t)slot * (size_t)slot_len;
  asm volatile("" : "+v"(x));
  const double* dist = a.dist;
  asm volatile("" : "+v"(dist));
  const double INF = __builtin_huge_val();

  for (int prob = slot; prob < n_prob; prob += n_slots) {
    const int ia = (unsigned)prob / (unsigned)a.Lb, ib = (unsigned)prob % (unsigned)a.Lb;
    const int a0 = a.a_off[ia], b0 = a.b_off[ib];
    const int n = __builtin_amdgcn_readfirstlane(a.a_off[ia + 1] - a0);
    const int m = __builtin_amdgcn_readfirstlane(a.b_off[ib + 1] - b0);
    if (n <= 0 || m <= 0) {                       // an empty list
      if (lane == 0) {
        a.val[prob] = INF;
        a.status[prob] = (n < 0 || m < 0) ? 4 : 0;
      }
      continue;
    }
    // the D indices; lists or indices the host checks should have refused: status 4
    bool bad = n > CAP || m > CAP || n * m > slot_len;
#pragma unroll
    for (int k = 0; k < NK; ++k) {
      const int e = lane + 64 * k;
      const int ri = e < n && !bad ? a.a_idx[a0 + e] : 0;
      const int cj = e < m && !bad ? a.b_idx[b0 + e] : 0;
      bad = bad || ri < 0 || ri >= a.Ua || cj < 0 || cj >= a.Ub;
      L.ri[e] = ri;
      L.cj[e] = cj;
    }
    if (__ballot(bad)) {
      if (lane == 0) {
        a.val[prob] = INF - INF;
        a.status[prob] = 4;
      }
      continue;
    }
    const int g = wm_gcd(n, m);
    const int sup = m / g, dem = n / g, T = n / g * m;
    // state: zero flow and potentials, full demands
    {
      uint4* xz = reinterpret_cast<uint4*>(x);
      const int n16 = (n * m + 7) >> 3;           // <= slot_len / 8
      for (int e = lane; e < n16; e += 64) xz[e] = make_uint4(0u, 0u, 0u, 0u);
    }
    // (entries past n / m are written like the others and never read: no per-entry predicates,
    // which the compiler would keep as 2 NK loop-invariant lane masks in scalar registers)
    unsigned pastS = 0u, pastT = 0u;              // bit k: the lane's k-th source / sink is past the end
#pragma unroll
    for (int k = 0; k < NK; ++k) {
      const int e = lane + 64 * k;
      L.p[e] = 0.0; L.pS[e] = 0;
      L.q[e] = 0.0; L.pT[e] = 0; L.t[e] = (uint16_t)dem;
      pastS |= (e < n ? 0u : 1u) << k;
      pastT |= (e < m ? 0u : 1u) << k;
    }
    wm_flow_fence();

    int status = 0;
    for (int r = 0; r < n && !status; ++r) {
      int s = sup;
      for (int it = 0; it < T && s > 0 && !status; ++it) {
        // ---- 1. Dijkstra from r
        double dS[NK], dT[NK];
        // (bit k: r is the lane's k-th source; opaque, or its NK tests would be hoisted out of
        // this loop into scalar registers as lane masks)
        unsigned isr = lane == (r & 63) ? 1u << (r >> 6) : 0u;
        asm volatile("" : "+v"(isr));
#pragma unroll
        for (int k = 0; k < NK; ++k) {
          dS[k] = (isr >> k) & 1u ? 0.0 : INF;
          dT[k] = INF;
        }
        unsigned vS = pastS, vT = pastT;             // visited (or absent)
        int tgt = -1;
        double delta = 0.0;
        for (int v = 0; v < n + m; ++v) {
          double d = INF;
          int id = WM_NONE;
#pragma unroll
          for (int k = 0; k < NK; ++k) {
            const int e = lane + 64 * k;
            if (!((vS >> k) & 1u) && dS[k] < d) { d = dS[k]; id = e; }
          }
#pragma unroll
          for (int k = 0; k < NK; ++k) {
            const int e = lane + 64 * k;
            if (!((vT >> k) & 1u) && dT[k] < d) { d = dT[k]; id = CAP + e; }
          }
          wm_argmin(d, id);
          if (id == WM_NONE) break;               // nothing reachable is left: no target
          if (id < CAP) {                         // a source: relax its unvisited sinks
            const int i = id;
            if (lane == (i & 63)) vS |= 1u << (i >> 6);
            const double pi = L.p[i];
            const double* drow = dist + (size_t)L.ri[i] * (size_t)a.ldd;
#pragma unroll
            for (int k = 0; k < NK; ++k) {
              // (a lane without an open sink here reads sink 0's entries and drops them: the
              // loads stay unpredicated and back to back)
              const int j = lane + 64 * k;
              const bool on = !((vT >> k) & 1u);
              const int jr = on ? j : 0;
              const double rc = (drow[L.cj[jr]] + pi) - L.q[jr];
              const double nd = d + (rc > 0.0 ? rc : 0.0);
              if (on && nd < dT[k]) { dT[k] = nd; L.pT[j] = (uint16_t)i; }
            }
          } else {
            const int j = id - CAP;
            if (wm_u(L.t[j]) > 0) {               // residual demand: the target
              tgt = j;
              delta = d;
              break;
            }
            if (lane == (j & 63)) vT |= 1u << (j >> 6);
            const double qj = L.q[j];
            const int cjj = L.cj[j];
            const uint16_t* xcol = x + j * n;
#pragma unroll
            for (int k = 0; k < NK; ++k) {
              const int i = lane + 64 * k;
              if (!((vS >> k) & 1u) && xcol[i] > 0) {
                const double rc = (dist[(size_t)L.ri[i] * (size_t)a.ldd + cjj] + L.p[i]) - qj;
                const double nd = d - (rc > 0.0 ? rc : 0.0);
                if (nd < dS[k]) { dS[k] = nd; L.pS[i] = (uint16_t)j; }
              }
            }
          }
        }
        if (tgt < 0) { status = 1; break; }
        // ---- 2. potentials
#pragma unroll
        for (int k = 0; k < NK; ++k) {
          const int e = lane + 64 * k;
          L.p[e] += dS[k] < delta ? dS[k] : delta;
          L.q[e] += dT[k] < delta ? dT[k] : delta;
        }
        // ---- 3. augment: every lane walks the chain (uniform reads), lane 0 stores
        const int tt = wm_u(L.t[tgt]);
        int amt = s < tt ? s : tt;
        bool open = true;
        int j = tgt;
        for (int h = 0; h < n + m && open; ++h) {
          const int i = wm_u(L.pT[j]);
          if (i == r) { open = false; break; }
          const int jj = wm_u(L.pS[i]);
          const int f = wm_u(x[jj * n + i]);
          amt = f < amt ? f : amt;
          j = jj;
        }
        if (open || amt <= 0) { status = 3; break; }
        open = true;
        j = tgt;
        for (int h = 0; h < n + m && open; ++h) {
          const int i = wm_u(L.pT[j]);
          const int f = x[j * n + i];
          if (lane == 0) x[j * n + i] = (uint16_t)(f + amt);
          if (i == r) { open = false; break; }
          const int jj = wm_u(L.pS[i]);
          const int fb = x[jj * n + i];
          if (lane == 0) x[jj * n + i] = (uint16_t)(fb - amt);
          j = jj;
        }
        if (lane == 0) L.t[tgt] = (uint16_t)(tt - amt);
        s -= amt;
        wm_flow_fence();
      }
      if (!status && s > 0) status = 2;
    }
    // ---- the value: the lane's rows summed in j order, the rows added in i order
    double rs[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) rs[k] = 0.0;
    for (int j = 0; j < m; ++j) {
      const int cjj = L.cj[j];
      const uint16_t* xcol = x + j * n;
#pragma unroll
      for (int k = 0; k < NK; ++k) {
        const int i = lane + 64 * k;
        if (!((pastS >> k) & 1u)) {
          const int f = xcol[i];
          if (f > 0) rs[k] = rs[k] + (double)f * dist[(size_t)L.ri[i] * (size_t)a.ldd + cjj];
        }
      }
    }
#pragma unroll
    for (int k = 0; k < NK; ++k)
      L.p[lane + 64 * k] = rs[k];
    double total = 0.0;
    for (int i = 0; i < n; ++i) total = total + L.p[i];
    if (lane == 0) {
      a.val[prob] = status ? INF - INF : total / (double)T;
      a.status[prob] = status;
    }
  }
}

inline int wm_cap(const GfkWmd* p) {
  if (p->cap) return p->cap;
  const int w = p->max_a > p->max_b ? p->max_a : p->max_b;
  return w <= WM_SMALL ? WM_SMALL : WM_MAX;
}

}  // namespace

extern "C" size_t gfk_wmd_dist_struct_size() { return sizeof(GfkWmdDist); }
extern "C" size_t gfk_wmd_struct_size() { return sizeof(GfkWmd); }

// the longest list gfk_wmd_solve takes
extern "C" int gfk_wmd_max_words() { return WM_MAX; }

// workgroups of a gfk_wmd_solve launch (cap: 0, 128 or 512 as in GfkWmd); -1: invalid
extern "C" int gfk_wmd_grid(int max_a, int max_b, int cap, int64_t n_prob, int max_grid) {
  if (max_a < 0 || max_b < 0 || max_a > WM_MAX || max_b > WM_MAX || n_prob < 0 ||
      n_prob >= ((int64_t)1 << 31) || max_grid < 0)
    return -1;
  if (cap != 0 && cap != WM_SMALL && cap != WM_MAX) return -1;
  const int w = max_a > max_b ? max_a : max_b;
  if (cap == 0) cap = w <= WM_SMALL ? WM_SMALL : WM_MAX;
  if (w > cap) return -1;
  int64_t grid = (n_prob + WM_WAVES - 1) / WM_WAVES;
  const int dflt = cap == WM_SMALL ? WM_GRID_SMALL : WM_GRID_LARGE;
  if (grid > dflt) grid = dflt;
  if (max_grid > 0 && grid > max_grid) grid = max_grid;
  return grid < 1 ? 1 : (int)grid;
}

// entries (uint16) of the flow workspace of that launch
extern "C" int64_t gfk_wmd_flow_len(int max_a, int max_b, int grid) {
  if (max_a < 0 || max_b < 0 || max_a > WM_MAX || max_b > WM_MAX || grid < 1) return -1;
  return (int64_t)grid * WM_WAVES * wm_slot_len(max_a, max_b);
}

// Host checks mirror the kernel's assumptions: Ua, Ub, dim >= 1 in an int, strides that hold a
// row.  Nothing is launched when a check fails.
extern "C" int gfk_wmd_dist(const GfkWmdDist* p, hipStream_t s) {
  if (!p) return -7;
  if (p->Ua < 1 || p->Ub < 1 || p->dim < 1 || p->max_grid < 0) return -5;
  if (p->lda < p->dim || p->ldb < p->dim || p->ldo < p->Ub) return -6;
  if (!p->a || !p->b || !p->out) return -7;
  const int64_t nta = (p->Ua + WD_T - 1) / WD_T, ntb = (p->Ub + WD_T - 1) / WD_T;
  if (nta * ntb >= ((int64_t)1 << 31)) return -6;
  const int n_tiles = (int)(nta * ntb);
  int grid = n_tiles < WD_GRID ? n_tiles : WD_GRID;
  if (p->max_grid > 0 && grid > p->max_grid) grid = p->max_grid;
  hipLaunchKernelGGL(gfk_wmd_dist_k, dim3(grid), dim3(WD_THREADS), 0, s, *p, (int)ntb, n_tiles);
  return (int)hipGetLastError();
}

// La, Lb >= 1 lists of at most max_a / max_b <= the instance's words each (the kernel refuses a
// longer list or an index outside D with status 4 instead of reading past its state), a flow
// workspace of gfk_wmd_flow_len entries for the grid of gfk_wmd_grid.
extern "C" int gfk_wmd_solve(const GfkWmd* p, hipStream_t s) {
  if (!p) return -7;
  if (p->La < 1 || p->Lb < 1 || p->Ua < 1 || p->Ub < 1 || p->ldd < p->Ub) return -6;
  const int64_t n_prob = (int64_t)p->La * p->Lb;
  const int grid = gfk_wmd_grid(p->max_a, p->max_b, p->cap, n_prob, p->max_grid);
  if (grid < 1) return -5;
  if (!p->dist || !p->a_off || !p->a_idx || !p->b_off || !p->b_idx || !p->flow || !p->val ||
      !p->status)
    return -7;
  if (((uintptr_t)p->flow & 15) || p->flow_len < gfk_wmd_flow_len(p->max_a, p->max_b, grid)) return -9;
  if (wm_cap(p) == WM_SMALL)
    hipLaunchKernelGGL(gfk_wmd_solve_k<WM_SMALL>, dim3(grid), dim3(WM_THREADS), 0, s, *p, (int)n_prob);
  else
    hipLaunchKernelGGL(gfk_wmd_solve_k<WM_MAX>, dim3(grid), dim3(WM_THREADS), 0, s, *p, (int)n_prob);
  return (int)hipGetLastError();
}
