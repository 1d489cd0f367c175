// optim.hip -- device-resident optimiser step (include/rmx.h rmx_optim_*): the reference's optimize() after
// the backward (ParRecModel.scala:439-478): per-id sums of the per-nonzero gradients (makeWeightsGrad /
// makeEmbeddingGrad, :293-328) pushed through SGD / Momentum / Adagrad / Adam, on the table rows and on mats.
//
// Sparse half, without float atomics (a store pass plus a per-destination sum pass through an inverted index):
//   1. stable LSD radix sort of (id, nonzero n) by id over the id bits V needs, 8 bits a pass (tile histogram,
//      exclusive scan in two launches, stable scatter ranked with wave ballots).  Ids outside [0, V) take the key V:
//      they sort last and are never addressed.
//   2. one 16-lane group per sorted position.  The group at the head of an id's list -- and, for lists longer
//      than 512, at every 512th position of it -- sums its (at most 512) gradient rows in ascending nonzero
//      order starting from the first term.  A list of <= 512 is updated there and then; the chunk sums of a
//      longer one go to a side buffer.
//   3. one group per long list adds its chunk sums in chunk order and updates the row.
// The order of every sum is fixed by the data alone, so results are bitwise repeatable whatever the launch
// geometry.  Dense half: one elementwise kernel over mats and its state, then the model's repack.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "rmx_internal.hpp"
#include "rmx_models.hpp"

namespace rmx {

namespace {

struct Hyper {
  int kind;
  float eta, a, b, eps;  // a: momentum / factor / beta, b: gamma
  float ia, ib;          // 1 - a, 1 - b
  float c1, c2;          // Adam: 1 - beta^t, 1 - gamma^t (host, double precision, rounded once)
};

// One parameter's update from its aggregated gradient g; s1 / s2: the values of its state slots, updated in place
// (the kinds that have none leave them alone).
__device__ __forceinline__ float opt_update(const Hyper& h, float p, float g, float& s1, float& s2) {
  switch (h.kind) {
    case RMX_OPTIM_SGD:
      return p - h.eta * g;
    case RMX_OPTIM_MOMENTUM:
      s1 = h.a * s1 + g;
      return p - h.eta * s1;
    case RMX_OPTIM_ADAGRAD:
      s1 = h.a * s1 + h.ia * (g * g);
      return p - h.eta * g / (sqrtf(s1) + h.eps);
    default:  // RMX_OPTIM_ADAM
      s1 = h.a * s1 + h.ia * g;
      s2 = h.b * s2 + h.ib * (g * g);
      return p - h.eta * (s1 / h.c1) / (sqrtf(s2 / h.c2) + h.eps);
  }
}

// a parameter with its state slots, loaded (slots the optimiser does not hold read as 0) and stored back
struct PVal {
  float p, s1, s2;
};
__device__ __forceinline__ PVal pv_load(const float* p, const float* s1, const float* s2, size_t i) {
  PVal v;
  v.p = p[i];
  v.s1 = s1 ? s1[i] : 0.f;
  v.s2 = s2 ? s2[i] : 0.f;
  return v;
}
__device__ __forceinline__ void pv_store(const PVal& v, float* p, float* s1, float* s2, size_t i) {
  p[i] = v.p;
  if (s1) s1[i] = v.s1;
  if (s2) s2[i] = v.s2;
}
// the same with the parameter at ip and its state at is (the [emb | w | pad] line rows of a shard partition: the
// state slots stay dense)
__device__ __forceinline__ PVal pv_load(const float* p, const float* s1, const float* s2, size_t ip, size_t is) {
  PVal v;
  v.p = p[ip];
  v.s1 = s1 ? s1[is] : 0.f;
  v.s2 = s2 ? s2[is] : 0.f;
  return v;
}
__device__ __forceinline__ void pv_store(const PVal& v, float* p, float* s1, float* s2, size_t ip, size_t is) {
  p[ip] = v.p;
  if (s1) s1[is] = v.s1;
  if (s2) s2[is] = v.s2;
}

// ------------------------------------------------------------------ radix sort ----
constexpr int kRsThreads = 256, kRsItems = 16, kRsTile = kRsThreads * kRsItems, kRsBins = 256;
constexpr int kChunkRows = 512;  // the split of a long list (a quarter of a wave's share of the rows)

template <bool FIRST>
__device__ __forceinline__ uint32_t rs_key(const int32_t* ids, const uint32_t* kin, int e, uint32_t V) {
  if (!FIRST) return kin[e];
  const int32_t id = ids[e];
  return (id >= 0 && (uint32_t)id < V) ? (uint32_t)id : V;
}

// hist[d * nb + tile] = elements of the tile whose digit is d (element e of a tile: base + i * 256 + thread)
template <bool FIRST>
__global__ __launch_bounds__(kRsThreads) void rs_hist_kernel(const int32_t* __restrict__ ids,
                                                            const uint32_t* __restrict__ kin, int n, int nb, int shift,
                                                            uint32_t V, uint32_t* __restrict__ hist) {
  __shared__ uint32_t h[kRsBins];
  h[threadIdx.x] = 0;
  __syncthreads();
  const int base = blockIdx.x * kRsTile;
#pragma unroll
  for (int i = 0; i < kRsItems; ++i) {
    const int e = base + i * kRsThreads + threadIdx.x;
    if (e < n) atomicAdd(&h[(rs_key<FIRST>(ids, kin, e, V) >> shift) & (kRsBins - 1)], 1u);  // integer, in LDS
  }
  __syncthreads();
  hist[(size_t)threadIdx.x * nb + blockIdx.x] = h[threadIdx.x];
}

// exclusive scan of a[0, n) in place, in two launches of n / 1024 blocks: the sums of the 1,024-element blocks,
// then every block scans its elements from the sum of the blocks before it
constexpr int kScanThreads = 256, kScanPer = 4, kScanBlock = kScanThreads * kScanPer;

__device__ __forceinline__ uint32_t block_sum(uint32_t v, uint32_t* lds) {  // 256 threads; lds [4]
  for (int d = 32; d > 0; d >>= 1) v += (uint32_t)__shfl_down((int)v, d, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  return lds[0] + lds[1] + lds[2] + lds[3];
}

__global__ __launch_bounds__(kScanThreads) void rs_scan_sums_kernel(const uint32_t* __restrict__ a, int n,
                                                                   uint32_t* __restrict__ bsum) {
  __shared__ uint32_t lds[4];
  const int base = blockIdx.x * kScanBlock;
  uint32_t v = 0;
#pragma unroll
  for (int i = 0; i < kScanPer; ++i) {
    const int e = base + i * kScanThreads + threadIdx.x;
    if (e < n) v += a[e];
  }
  v = block_sum(v, lds);
  if (threadIdx.x == 0) bsum[blockIdx.x] = v;
}

__global__ __launch_bounds__(kScanThreads) void rs_scan_apply_kernel(uint32_t* __restrict__ a, int n,
                                                                    const uint32_t* __restrict__ bsum) {
  __shared__ uint32_t lds[4];
  __shared__ uint32_t part[kScanThreads];
  uint32_t before = 0;
  for (int b = threadIdx.x; b < (int)blockIdx.x; b += kScanThreads) before += bsum[b];
  before = block_sum(before, lds);
  const int e0 = blockIdx.x * kScanBlock + threadIdx.x * kScanPer;  // kScanPer consecutive elements a thread
  uint32_t v[kScanPer], sum = 0;
#pragma unroll
  for (int i = 0; i < kScanPer; ++i) {
    v[i] = e0 + i < n ? a[e0 + i] : 0u;
    sum += v[i];
  }
  part[threadIdx.x] = sum;
  __syncthreads();
  for (int d = 1; d < kScanThreads; d <<= 1) {
    const uint32_t add = threadIdx.x >= (unsigned)d ? part[threadIdx.x - d] : 0u;
    __syncthreads();
    part[threadIdx.x] += add;
    __syncthreads();
  }
  uint32_t run = before + part[threadIdx.x] - sum;
#pragma unroll
  for (int i = 0; i < kScanPer; ++i) {
    if (e0 + i < n) a[e0 + i] = run;
    run += v[i];
  }
}

// stable scatter of one tile: an element's place among its digit's elements is (items before it in the tile
// order (i, wave, lane)) + the scanned count of the tiles before
template <bool FIRST>
__global__ __launch_bounds__(kRsThreads) void rs_scatter_kernel(const int32_t* __restrict__ ids,
                                                               const uint32_t* __restrict__ kin,
                                                               const uint32_t* __restrict__ vin,
                                                               uint32_t* __restrict__ kout, uint32_t* __restrict__ vout,
                                                               const uint32_t* __restrict__ offs, int n, int nb,
                                                               int shift, uint32_t V) {
  __shared__ uint32_t cnt[kRsItems][kRsThreads / 64][kRsBins];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  for (int i = tid; i < kRsItems * (kRsThreads / 64) * kRsBins; i += kRsThreads) (&cnt[0][0][0])[i] = 0;
  __syncthreads();
  const int base = blockIdx.x * kRsTile;
  uint32_t key[kRsItems], val[kRsItems], rank[kRsItems];
#pragma unroll
  for (int i = 0; i < kRsItems; ++i) {
    const int e = base + i * kRsThreads + tid;
    const bool valid = e < n;
    key[i] = valid ? rs_key<FIRST>(ids, kin, e, V) : 0xFFFFFFFFu;
    val[i] = valid ? (FIRST ? (uint32_t)e : vin[e]) : 0u;
    const uint32_t d = (key[i] >> shift) & (kRsBins - 1);
    unsigned long long same = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = (d >> b) & 1u;
      const unsigned long long bal = __ballot(bit);
      same &= bit ? bal : ~bal;
    }
    rank[i] = (uint32_t)__popcll(same & ((1ull << lane) - 1ull));
    if (valid && rank[i] == 0) cnt[i][w][d] = (uint32_t)__popcll(same);
  }
  __syncthreads();
  {
    uint32_t run = offs[(size_t)tid * nb + blockIdx.x];  // thread = digit
    for (int i = 0; i < kRsItems; ++i)
      for (int ww = 0; ww < kRsThreads / 64; ++ww) {
        const uint32_t c = cnt[i][ww][tid];
        cnt[i][ww][tid] = run;
        run += c;
      }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < kRsItems; ++i) {
    const int e = base + i * kRsThreads + tid;
    if (e < n) {
      const uint32_t dst = cnt[i][w][(key[i] >> shift) & (kRsBins - 1)] + rank[i];
      if (dst < (uint32_t)n) {  // (always: the histogram counts the same keys)
        kout[dst] = key[i];
        vout[dst] = val[i];
      }
    }
  }
}

// ------------------------------------------------------------ sparse update ----
struct TabArgs {
  const uint32_t* sk;  // sorted keys [n]
  const uint32_t* sv;  // their nonzeros, ascending within a key
  int n;
  uint32_t V;
  int k;               // columns of the table
  const float* gw;     // [n] or null
  const float* ge;     // [n][k] or null
  float* w;            // [V]
  float* emb;          // [V][k]
  float* line;         // [V][32] line copy of a k = 16 table, or null
  float *ws1, *ws2, *es1, *es2;
  float* part;         // [2 * windows][k + 1]
  int32_t* long_head;  // [windows]
  Hyper h;
  static constexpr bool kLines = false;
};
// the same for the [emb k | w | pad] line rows of a shard partition (w: the w slot of row 0): the parameters
// take the row stride rs, the state slots stay dense.  A type of its own, so that the replicated table's
// kernels keep their arguments and their code.
struct LineArgs : TabArgs {
  int rs;  // row stride in floats
  static constexpr bool kLines = true;
};

// Adds the gradient rows of 8 list positions, in order, to se / sw: position r0 + r of a 16-position window is
// nonzero idx16 of lane r0 + r, and counts while r0 + r < left.  init: the window's position 0 starts the sums.
// Eight rows in flight a group keep the kernel's registers (their addresses above all) at 8 waves a SIMD's
// worth: what hides the latency of these dependent random reads is occupancy.
__device__ __forceinline__ void add8(const TabArgs& a, uint32_t idx16, int r0, int left, int col, bool act, bool do_w,
                                     bool init, float& se, float& sw) {
  float ve[8], vw[8];
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const uint32_t nz = (uint32_t)__shfl((int)idx16, r0 + r, 16);
    const bool on = r0 + r < left;
    ve[r] = (on && act) ? a.ge[(size_t)nz * a.k + col] : 0.f;
    vw[r] = (on && do_w) ? a.gw[nz] : 0.f;
  }
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const bool on = r0 + r < left;
    if (init && r == 0) {
      se = ve[0];
      sw = vw[0];
    } else {
      se = on ? se + ve[r] : se;  // (no + 0.f for the lanes past the end: it would turn a -0 sum into +0)
      sw = on ? sw + vw[r] : sw;
    }
  }
}

// fp32 sums over the list positions [p, p + cnt): se of ge[sv[q]][col] (lanes with act), sw of gw[sv[q]], each in
// ascending q starting from the first term.  The 16 lanes of a group run it together (cnt is theirs alike);
// sv16: lane r holds sv[p + r] (whatever past the list's end).
__device__ __forceinline__ void sum_list(const TabArgs& a, int p, int cnt, int gl, uint32_t sv16, int col, bool act,
                                         bool do_w, float& se, float& sw) {
  add8(a, sv16, 0, cnt, col, act, do_w, true, se, sw);
  if (cnt > 8) add8(a, sv16, 8, cnt, col, act, do_w, false, se, sw);
  if (cnt <= 16) return;
  // the rest of a longer list, 16 positions a turn, their nonzeros loaded a turn ahead
  const int end = p + cnt;
  uint32_t nxt = a.sv[min(p + 16 + gl, end - 1)];
  for (int q0 = p + 16; q0 < end; q0 += 16) {
    const int left = end - q0;  // >= 1
    const uint32_t mine = nxt;
    if (q0 + 16 < end) nxt = a.sv[min(q0 + 16 + gl, end - 1)];
    add8(a, mine, 0, left, col, act, do_w, false, se, sw);
    if (left > 8) add8(a, mine, 8, left, col, act, do_w, false, se, sw);
  }
}

// the parameters of row `key` with their state, loaded and stored (A: TabArgs or LineArgs, fixed at compile time)
template <class A>
__device__ __forceinline__ PVal load_emb(const A& a, uint32_t key, int col) {
  if constexpr (A::kLines) return pv_load(a.emb, a.es1, a.es2, (size_t)key * a.rs + col, (size_t)key * a.k + col);
  else return pv_load(a.emb, a.es1, a.es2, (size_t)key * a.k + col);
}
template <class A>
__device__ __forceinline__ PVal load_w(const A& a, uint32_t key) {
  if constexpr (A::kLines) return pv_load(a.w, a.ws1, a.ws2, (size_t)key * a.rs, key);
  else return pv_load(a.w, a.ws1, a.ws2, key);
}
template <class A>
__device__ __forceinline__ void store_emb(const A& a, const PVal& v, uint32_t key, int col) {
  if constexpr (A::kLines) pv_store(v, a.emb, a.es1, a.es2, (size_t)key * a.rs + col, (size_t)key * a.k + col);
  else pv_store(v, a.emb, a.es1, a.es2, (size_t)key * a.k + col);
}
template <class A>
__device__ __forceinline__ void store_w(const A& a, const PVal& v, uint32_t key) {
  if constexpr (A::kLines) pv_store(v, a.w, a.ws1, a.ws2, (size_t)key * a.rs, key);
  else pv_store(v, a.w, a.ws1, a.ws2, key);
}

// the row of id `key` from its loaded values: column col of the embedding (lanes with act) and, lane 0 of the
// group, the weight; the line copy gets the new values too
template <class A>
__device__ __forceinline__ void finish_row(const A& a, uint32_t key, int gl, int col, bool act, bool do_w,
                                           PVal pe, PVal pw, float ge_sum, float gw_sum) {
  if (act) {
    pe.p = opt_update(a.h, pe.p, ge_sum, pe.s1, pe.s2);
    store_emb(a, pe, key, col);
    if (a.line) a.line[(size_t)key * 32 + col] = pe.p;
  }
  if (do_w && gl == 0) {
    pw.p = opt_update(a.h, pw.p, gw_sum, pw.s1, pw.s2);
    store_w(a, pw, key);
    if (a.line) a.line[(size_t)key * 32 + 16] = pw.p;
  }
}

// K16: the table has 16 columns, lane j of a group owns column j; else column chunks of 16 in turn.
// Everything a group needs to place itself comes from one round of loads: its key, the key before, the 16 keys
// after (one a lane) and the 16 nonzeros from its position on.
template <bool K16, class A>
__global__ __launch_bounds__(256) void tab_update_kernel(A a) {
  const size_t gp = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
  const int gl = threadIdx.x & 15;
  if (gp >= (size_t)a.n) return;
  const int p = (int)gp;
  const uint32_t key = a.sk[p];
  const uint32_t prev = p > 0 ? a.sk[p - 1] : 0xFFFFFFFFu;  // (keys are <= V < 2^31)
  const uint32_t next = p + 1 + gl < a.n ? a.sk[p + 1 + gl] : 0xFFFFFFFFu;
  const uint32_t sv16 = a.sv[min(p + gl, a.n - 1)];
  const uint32_t m16 = (uint32_t)(__ballot(next == key) >> (threadIdx.x & 48)) & 0xFFFFu;  // this group's 16 bits
  if (key >= a.V) return;  // an id outside the table
  const bool head = prev != key;
  if (!head) {
    // a later chunk of a long list starts here iff this position is a multiple of 512 past the list's head
    if (p < kChunkRows || a.sk[p - kChunkRows] != key) return;
    int lo = 0, hi = p - kChunkRows;  // first position of key: in [0, p - 512]
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (a.sk[mid] < key) lo = mid + 1; else hi = mid;
    }
    if ((p - lo) % kChunkRows) return;
  }
  // rows of this chunk: positions [p, p + cnt) holding key, cnt <= 512
  const int lim = min(a.n, p + kChunkRows);
  int cnt;
  if (m16 != 0xFFFFu) {
    cnt = __ffs((int)~m16);  // 1 + the run of matching keys after p
  } else {                   // p + 1 .. p + 16 hold key: first position in [p + 17, lim] that does not
    int lo = p + 17, hi = lim;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (a.sk[mid] == key) lo = mid + 1; else hi = mid;
    }
    cnt = lo - p;
  }
  const bool more = lim < a.n && cnt == kChunkRows && a.sk[lim] == key;
  const bool direct = head && !more;
  const int ke = a.ge ? a.k : 0;
  const bool has_w = a.gw != nullptr;
  const int win = p / kChunkRows;
  float* prow = a.part + (size_t)(2 * win + (head ? 0 : 1)) * (a.k + 1);
  const int nch = K16 ? 1 : max(1, (ke + 15) / 16);
  for (int c = 0; c < nch; ++c) {
    const int col = c * 16 + gl;
    const bool act = col < ke;
    const bool do_w = has_w && c == 0;
    PVal pe{}, pw{};  // the row's old values, in flight while the gradient rows are summed
    if (direct && act) pe = load_emb(a, key, col);
    if (direct && do_w) pw = load_w(a, key);
    float se, sw;
    sum_list(a, p, cnt, gl, sv16, col, act, do_w, se, sw);
    if (direct) {
      finish_row(a, key, gl, col, act, do_w, pe, pw, se, sw);
    } else {
      if (act) prow[col] = se;
      if (do_w && gl == 0) prow[a.k] = sw;
    }
  }
  if (!direct && head && gl == 0) a.long_head[win] = p;
}

// lists longer than 512: the chunk sums added in chunk order, then the update; one group per 512-window
template <bool K16, class A>
__global__ __launch_bounds__(256) void tab_long_kernel(A a, int windows) {
  const int win = (int)((blockIdx.x * (unsigned)blockDim.x + threadIdx.x) >> 4);
  const int gl = threadIdx.x & 15;
  if (win >= windows) return;
  const int p = a.long_head[win];
  if (p < 0) return;
  const uint32_t key = a.sk[p];
  const int ke = a.ge ? a.k : 0;
  const bool has_w = a.gw != nullptr;
  const int nch = K16 ? 1 : max(1, (ke + 15) / 16);
  const size_t ld = (size_t)a.k + 1;
  for (int c = 0; c < nch; ++c) {
    const int col = c * 16 + gl;
    const bool act = col < ke;
    const bool do_w = has_w && c == 0;
    const float* r0 = a.part + (size_t)(2 * win) * ld;
    float se = act ? r0[col] : 0.f, sw = do_w ? r0[a.k] : 0.f;
    for (int q = p + kChunkRows; q < a.n && a.sk[q] == key; q += kChunkRows) {
      const float* r = a.part + (size_t)(2 * (q / kChunkRows) + 1) * ld;
      if (act) se += r[col];
      if (do_w) sw += r[a.k];
    }
    PVal pe{}, pw{};
    if (act) pe = load_emb(a, key, col);
    if (do_w) pw = load_w(a, key);
    finish_row(a, key, gl, col, act, do_w, pe, pw, se, sw);
  }
}

// ------------------------------------------------------------- dense update ----
__global__ __launch_bounds__(256) void dense_update_kernel(int64_t n, float* __restrict__ p, const float* __restrict__ g,
                                                          float* s1, float* s2, Hyper h) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  PVal v = pv_load(p, s1, s2, (size_t)i);
  v.p = opt_update(h, v.p, g[i], v.s1, v.s2);
  pv_store(v, p, s1, s2, (size_t)i);
}
// four parameters a thread (n4 float4 groups; every pointer 16-byte aligned)
__global__ __launch_bounds__(256) void dense_update4_kernel(int64_t n4, float* __restrict__ p,
                                                           const float* __restrict__ g, float* s1, float* s2, Hyper h) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n4) return;
  float4 pv = reinterpret_cast<float4*>(p)[i];
  const float4 gv = reinterpret_cast<const float4*>(g)[i];
  float4 a = s1 ? reinterpret_cast<float4*>(s1)[i] : make_float4(0.f, 0.f, 0.f, 0.f);
  float4 b = s2 ? reinterpret_cast<float4*>(s2)[i] : make_float4(0.f, 0.f, 0.f, 0.f);
  pv.x = opt_update(h, pv.x, gv.x, a.x, b.x);
  pv.y = opt_update(h, pv.y, gv.y, a.y, b.y);
  pv.z = opt_update(h, pv.z, gv.z, a.z, b.z);
  pv.w = opt_update(h, pv.w, gv.w, a.w, b.w);
  reinterpret_cast<float4*>(p)[i] = pv;
  if (s1) reinterpret_cast<float4*>(s1)[i] = a;
  if (s2) reinterpret_cast<float4*>(s2)[i] = b;
}

// The values the model keeps on the host, gathered for one small copy: hv[0] the global bias after its update,
// [1] bo, [2 + l] sum_d w_l[d] and [2 + kMaxFusedCross + l] beta_l of DCN, [2 + 2 kMaxFusedCross] sum_d
// W_out[d] (the double-precision sequential sums of model_load_mats, bit for bit), [last] the step's loss.
struct HostValArgs {
  float beta;
  const float* g_bias;
  float* bs;  // [2] bias state slots
  const float* mats;
  int64_t bo_off, cross_w_off, cross_b_off, wo_x_off;  // -1: none
  int L, D;
  const float* loss;
  Hyper h;
};
__global__ void host_vals_kernel(HostValArgs a, float* __restrict__ hv) {
  const int t = threadIdx.x;
  if (t == 0) {
    float beta = a.beta;
    if (a.g_bias) {
      float s1 = a.bs[0], s2 = a.bs[1];
      beta = opt_update(a.h, beta, a.g_bias[0], s1, s2);
      a.bs[0] = s1;
      a.bs[1] = s2;
    }
    hv[0] = beta;
  }
  if (t == 1) hv[1] = a.bo_off >= 0 ? a.mats[a.bo_off] : 0.f;
  if (t >= 2 && t < 2 + a.L) {
    const int l = t - 2;
    double ws = 0.0;
    for (int d = 0; d < a.D; ++d) ws += a.mats[a.cross_w_off + (int64_t)l * a.D + d];
    hv[2 + l] = (float)ws;
    hv[2 + kMaxFusedCross + l] = a.mats[a.cross_b_off + l];
  }
  if (t == 2 + kMaxFusedCross && a.L > 0) {
    double wo = 0.0;
    for (int d = 0; d < a.D; ++d) wo += a.mats[a.wo_x_off + d];
    hv[2 + 2 * kMaxFusedCross] = (float)wo;
  }
  if (t == 3 + kMaxFusedCross) hv[kOptimHostVals - 1] = a.loss ? a.loss[0] : 0.f;
}

// every buffer of the optimiser holds at least 4 elements
constexpr size_t kMinElems = 4;

int id_bits(int64_t V) {  // bits of the largest key, V itself (the key of an id outside the table)
  int b = 1;
  while ((V >> b) != 0) ++b;
  return b;
}

int ensure_scratch(rmx_optim& o, int64_t nnz) {
  if (nnz <= o.cap_nnz) return RMX_OK;
  RMX_HIP(hipDeviceSynchronize());
  o.cap_nnz = 0;
  const size_t tiles = (size_t)((nnz + kRsTile - 1) / kRsTile), windows = (size_t)(nnz / kChunkRows + 1);
  int st = RMX_OK;
  for (int i = 0; i < 2 && !st; ++i) {
    st = o.keys[i].alloc((size_t)nnz, "rmx_optim", kMinElems);
    if (!st) st = o.vals[i].alloc((size_t)nnz, "rmx_optim", kMinElems);
  }
  if (!st) st = o.hist.alloc(tiles * kRsBins, "rmx_optim", kMinElems);
  if (!st) st = o.bsum.alloc(tiles * kRsBins / kScanBlock + 1, "rmx_optim", kMinElems);
  if (!st) st = o.part.alloc(2 * windows * ((size_t)o.k + 1), "rmx_optim", kMinElems);
  if (!st) st = o.long_head.alloc(windows, "rmx_optim", kMinElems);
  if (st) return st;
  o.cap_nnz = nnz;
  return RMX_OK;
}

template <bool FIRST>
int sort_pass(hipStream_t s, const int32_t* ids, const uint32_t* kin, const uint32_t* vin, uint32_t* kout,
              uint32_t* vout, uint32_t* hist, uint32_t* bsum, int n, int shift, uint32_t V) {
  const int nb = (n + kRsTile - 1) / kRsTile;
  hipLaunchKernelGGL(rs_hist_kernel<FIRST>, dim3(nb), dim3(kRsThreads), 0, s, ids, kin, n, nb, shift, V, hist);
  const int nh = nb * kRsBins, nsb = (nh + kScanBlock - 1) / kScanBlock;
  hipLaunchKernelGGL(rs_scan_sums_kernel, dim3(nsb), dim3(kScanThreads), 0, s, hist, nh, bsum);
  hipLaunchKernelGGL(rs_scan_apply_kernel, dim3(nsb), dim3(kScanThreads), 0, s, hist, nh, bsum);
  hipLaunchKernelGGL(rs_scatter_kernel<FIRST>, dim3(nb), dim3(kRsThreads), 0, s, ids, kin, vin, kout, vout, hist, n, nb,
                     shift, V);
  RMX_HIP(hipGetLastError());
  return RMX_OK;
}

Hyper make_hyper(const rmx_optim& o, int64_t step) {
  Hyper h{};
  h.kind = o.kind;
  h.eta = (float)o.eta;
  h.a = (float)o.a;
  h.b = (float)o.b;
  h.eps = (float)o.eps;
  h.ia = (float)(1.0 - o.a);
  h.ib = (float)(1.0 - o.b);
  h.c1 = (float)(1.0 - std::pow(o.a, (double)step));
  h.c2 = (float)(1.0 - std::pow(o.b, (double)step));
  return h;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

int optim_alloc(rmx_optim& o) {
  const rmx_model& m = *o.m;
  const size_t rows = (size_t)o.rows * o.nparts;  // the table's V, or every partition held here
  RMX_HIP(hipSetDevice(m.ctx->device));
  int st = RMX_OK;
  for (int i = 0; i < o.nslots && !st; ++i) {
    if (o.upd_w) {
      if ((st = o.w_s[i].alloc(rows, "rmx_optim", kMinElems))) break;
      RMX_HIP(hipMemsetAsync(o.w_s[i], 0, sizeof(float) * rows, m.ctx->stream));
    }
    if (o.upd_e && o.k > 0) {
      if ((st = o.e_s[i].alloc(rows * o.k, "rmx_optim", kMinElems))) break;
      RMX_HIP(hipMemsetAsync(o.e_s[i], 0, sizeof(float) * rows * o.k, m.ctx->stream));
    }
    if (m.mats_len > 0) {
      if ((st = o.m_s[i].alloc((size_t)m.mats_len, "rmx_optim", kMinElems))) break;
      RMX_HIP(hipMemsetAsync(o.m_s[i], 0, sizeof(float) * m.mats_len, m.ctx->stream));
    }
  }
  if (!st) st = o.b_s.alloc(2, "rmx_optim", kMinElems);
  if (!st) st = o.hv.alloc(kOptimHostVals, "rmx_optim", kMinElems);
  if (st) return st;
  RMX_HIP(hipMemsetAsync(o.b_s, 0, sizeof(float) * 2, m.ctx->stream));
  RMX_HIP(hipStreamSynchronize(m.ctx->stream));
  return RMX_OK;
}

// The buffers go with the object at the caller's delete, after the synchronisation here.
void optim_release(rmx_optim& o) {
  if (o.m && o.m->ctx) {
    (void)hipSetDevice(o.m->ctx->device);
    (void)hipDeviceSynchronize();
  }
}

int optim_ensure_grads(rmx_optim& o, int64_t nnz) {
  int st = RMX_OK;
  if (!o.g_b) {
    st = o.g_b.alloc(2, "rmx_optim", kMinElems);
    if (!st && o.m->mats_len > 0) st = o.g_m.alloc((size_t)o.m->mats_len, "rmx_optim", kMinElems);
    if (st) return st;
  }
  if (nnz <= o.g_nnz) return RMX_OK;
  RMX_HIP(hipDeviceSynchronize());
  o.g_w.reset();
  o.g_e.reset();
  o.g_nnz = 0;
  if (o.upd_w) st = o.g_w.alloc((size_t)nnz, "rmx_optim", kMinElems);
  if (!st && o.upd_e) st = o.g_e.alloc((size_t)nnz * std::max(o.k, 1), "rmx_optim", kMinElems);
  if (st) return st;
  o.g_nnz = nnz;
  return RMX_OK;
}

// does a step on these groups change a value the model keeps on the host?
static bool optim_host_values(const rmx_optim& o, bool bias, bool mats) {
  const rmx_model& m = *o.m;
  return bias || (mats && (m.has_bo || (m.type == RMX_MODEL_DCN && m.cross_depth <= kMaxFusedCross)));
}

__global__ __launch_bounds__(256) void plane_sum_kernel(int N, int64_t len, const float* __restrict__ planes,
                                                       float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= len) return;
  float v = planes[i];
  for (int r = 1; r < N; ++r) v += planes[(int64_t)r * len + i];
  out[i] = v;
}

int optim_sum_planes(hipStream_t s, int N, int64_t len, const float* planes, float* out) {
  if (len <= 0) return RMX_OK;
  hipLaunchKernelGGL(plane_sum_kernel, dim3((unsigned)((len + 255) / 256)), dim3(256), 0, s, N, len, planes, out);
  RMX_HIP(hipGetLastError());
  return RMX_OK;
}

int optim_bucket_sort(rmx_optim& o, hipStream_t s, int64_t n, const int32_t* keys, int nkeys) {
  if (n <= 0) return RMX_OK;
  if (nkeys >= kRsBins || n >= (int64_t(1) << 31) - kRsTile) {
    set_error("rmx_optim_apply: batch * nFields must fit int32");
    return RMX_E_INVALID;
  }
  if (int st = ensure_scratch(o, n)) return st;
  return sort_pass<true>(s, keys, nullptr, nullptr, o.keys[0], o.vals[0], o.hist, o.bsum, (int)n, 0, (uint32_t)nkeys);
}

int optim_sparse_update(rmx_optim& o, hipStream_t s, int64_t nnz, const int32_t* ids, const SparseRows& t,
                        const float* g_w, const float* g_emb) {
  if (nnz >= (int64_t(1) << 31) - kRsTile) {
    set_error("rmx_optim_apply: batch * nFields must fit int32");
    return RMX_E_INVALID;
  }
  const Hyper h = make_hyper(o, o.steps + 1);
  int st;
  if ((g_w || g_emb) && nnz > 0) {
    if ((st = ensure_scratch(o, nnz))) return st;
    const int n = (int)nnz;
    const uint32_t V = (uint32_t)t.V;
    const int passes = (id_bits(t.V) + 7) / 8;
    int cur = 0;
    for (int pass = 0; pass < passes; ++pass) {
      if (pass == 0)
        st = sort_pass<true>(s, ids, nullptr, nullptr, o.keys[0], o.vals[0], o.hist, o.bsum, n, 0, V);
      else
        st = sort_pass<false>(s, nullptr, o.keys[cur], o.vals[cur], o.keys[cur ^ 1], o.vals[cur ^ 1], o.hist, o.bsum, n,
                              8 * pass, V);
      if (st) return st;
      if (pass > 0) cur ^= 1;
    }
    const int windows = n / kChunkRows + 1;
    RMX_HIP(hipMemsetAsync(o.long_head, 0xFF, sizeof(int32_t) * windows, s));
    LineArgs a{};
    a.sk = o.keys[cur];
    a.sv = o.vals[cur];
    a.n = n;
    a.V = V;
    a.k = t.k;
    a.gw = g_w;
    a.ge = g_emb;
    a.w = t.w;
    a.emb = t.emb;
    a.rs = t.rs;
    a.line = t.line;
    a.ws1 = t.ws[0];
    a.ws2 = t.ws[1];
    a.es1 = t.es[0];
    a.es2 = t.es[1];
    a.part = o.part;
    a.long_head = o.long_head;
    a.h = h;
    const unsigned gA = (unsigned)(((int64_t)n * 16 + 255) / 256), gB = (unsigned)(((int64_t)windows * 16 + 255) / 256);
    if (t.rs > 0) {  // a shard partition's line rows
      if (t.k == 16) {
        hipLaunchKernelGGL((tab_update_kernel<true, LineArgs>), dim3(gA), dim3(256), 0, s, a);
        hipLaunchKernelGGL((tab_long_kernel<true, LineArgs>), dim3(gB), dim3(256), 0, s, a, windows);
      } else {
        hipLaunchKernelGGL((tab_update_kernel<false, LineArgs>), dim3(gA), dim3(256), 0, s, a);
        hipLaunchKernelGGL((tab_long_kernel<false, LineArgs>), dim3(gB), dim3(256), 0, s, a, windows);
      }
    } else if (t.k == 16) {
      hipLaunchKernelGGL((tab_update_kernel<true, TabArgs>), dim3(gA), dim3(256), 0, s, a);
      hipLaunchKernelGGL((tab_long_kernel<true, TabArgs>), dim3(gB), dim3(256), 0, s, a, windows);
    } else {
      hipLaunchKernelGGL((tab_update_kernel<false, TabArgs>), dim3(gA), dim3(256), 0, s, a);
      hipLaunchKernelGGL((tab_long_kernel<false, TabArgs>), dim3(gB), dim3(256), 0, s, a, windows);
    }
    RMX_HIP(hipGetLastError());
  }
  return RMX_OK;
}

int optim_dense_update(rmx_optim& o, hipStream_t s, const float* g_bias, const float* g_mats, const float* loss_dev,
                       float* loss, bool sync) {
  rmx_model& m = *o.m;
  if (m.mats_len <= 0) g_mats = nullptr;
  const Hyper h = make_hyper(o, o.steps + 1);
  int st;
  if (g_mats) {
    const int64_t n = m.mats_len;
    if (aligned16(g_mats)) {
      const int64_t n4 = n / 4;
      if (n4 > 0)
        hipLaunchKernelGGL(dense_update4_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, n4, m.mats_dev,
                           g_mats, o.m_s[0], o.m_s[1], h);
      if (n > 4 * n4)
        hipLaunchKernelGGL(dense_update_kernel, dim3(1), dim3(256), 0, s, n - 4 * n4, m.mats_dev + 4 * n4,
                           g_mats + 4 * n4, o.m_s[0] ? o.m_s[0] + 4 * n4 : nullptr,
                           o.m_s[1] ? o.m_s[1] + 4 * n4 : nullptr, h);
    } else {
      hipLaunchKernelGGL(dense_update_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, n, m.mats_dev, g_mats,
                         o.m_s[0], o.m_s[1], h);
    }
    RMX_HIP(hipGetLastError());
    if ((st = model_repack(m, s))) return st;
  }
  o.steps += 1;
  if (!sync && !optim_host_values(o, g_bias != nullptr, g_mats != nullptr)) return RMX_OK;
  HostValArgs hv{};
  hv.beta = m.beta;
  hv.g_bias = g_bias;
  hv.bs = o.b_s;
  hv.mats = m.mats_dev;
  hv.bo_off = m.has_bo ? m.bo_off : -1;
  const bool dcn = m.type == RMX_MODEL_DCN && m.cross_depth <= kMaxFusedCross;
  hv.cross_w_off = m.cross_w_off;
  hv.cross_b_off = m.cross_b_off;
  hv.wo_x_off = m.wo_x_off;
  hv.L = dcn ? m.cross_depth : 0;
  hv.D = m.F * m.k;
  hv.loss = loss_dev;
  hv.h = h;
  hipLaunchKernelGGL(host_vals_kernel, dim3(1), dim3(64), 0, s, hv, o.hv);
  RMX_HIP(hipGetLastError());
  float host[kOptimHostVals];
  RMX_HIP(hipMemcpyAsync(host, o.hv, sizeof(host), hipMemcpyDeviceToHost, s));
  RMX_HIP(hipStreamSynchronize(s));
  if (g_bias) m.beta = host[0];
  if (g_mats) {
    if (m.has_bo) m.bo = host[1];
    for (int l = 0; l < hv.L; ++l) {
      m.cross_scalars.wsum[l] = host[2 + l];
      m.cross_scalars.beta[l] = host[2 + kMaxFusedCross + l];
    }
    if (hv.L > 0) m.cross_scalars.wo_sum = host[2 + 2 * kMaxFusedCross];
  }
  if (loss) *loss = host[kOptimHostVals - 1];
  return RMX_OK;
}

int optim_apply(rmx_optim& o, hipStream_t s, int32_t B, const int32_t* ids, const float* g_bias, const float* g_w,
                const float* g_emb, const float* g_mats, const float* loss_dev, float* loss, bool sync) {
  rmx_table& t = *o.t;
  if (!o.upd_w) g_w = nullptr;
  if (!o.upd_e || t.k <= 0) g_emb = nullptr;
  SparseRows r;
  r.V = t.V;
  r.k = t.k;
  r.w = (float*)t.w.get();
  r.emb = (float*)t.emb.get();
  r.line = t.line;
  for (int i = 0; i < 2; ++i) {
    r.ws[i] = o.w_s[i];
    r.es[i] = o.e_s[i];
  }
  if (int st = optim_sparse_update(o, s, (int64_t)B * o.m->F, ids, r, g_w, g_emb)) return st;
  return optim_dense_update(o, s, g_bias, g_mats, loss_dev, loss, sync);
}

namespace {

// the checks of the state row calls, all before any device call: the shared range checks, then the slot and the
// parts this optimiser holds state for
int state_rows_check(const char* who, const rmx_optim* o, int slot, int64_t id0, int64_t n, const float* weights,
                     const float* embedding, int layout, int64_t ld) {
  const int64_t V = !o ? 0 : o->sh ? shard_num_rows(o->sh) : o->rows;
  int st = rows_check(who, o, V, id0, n, layout, ld);
  if (st) return st;
  if (slot < 0 || slot >= o->nslots) {
    set_error(std::string(who) + ": slot " + std::to_string(slot) + ": this optimiser kind has " +
              std::to_string(o->nslots) + " state slot(s)");
    return RMX_E_INVALID;
  }
  if (weights && !o->w_s[slot]) {
    set_error(std::string(who) + ": weights: the optimiser holds no first-order state (DNN)");
    return RMX_E_INVALID;
  }
  if (embedding && !o->e_s[slot]) {
    set_error(std::string(who) + ": embedding: the optimiser holds no embedding state (LR)");
    return RMX_E_INVALID;
  }
  return RMX_OK;
}

int table_state_rows(rmx_optim& o, int slot, bool up, int64_t id0, int64_t n, float* weights, float* embedding,
                     int layout, int64_t ld, uint8_t* owned, int64_t* count) {
  std::lock_guard<std::mutex> lk(o.m->mu);
  RowSpace sp;
  sp.ctx = o.t->ctx;
  sp.io = &o.t->io;
  sp.op = owner_perm_of(0, o.rows);
  sp.N = 1;
  sp.k = o.k;
  RowTarget tg;
  tg.emb = o.e_s[slot];
  tg.w = o.w_s[slot];
  tg.es = o.k;
  return up ? rows_upload(sp, &tg, 1, id0, n, weights, embedding, layout, ld, count)
            : rows_download(sp, &tg, 1, id0, n, weights, embedding, layout, ld, owned, count);
}

int state_dense_check(const char* who, const rmx_optim* o, int slot) {
  if (!o) {
    set_error(std::string(who) + ": the optimiser is NULL");
    return RMX_E_INVALID;
  }
  if (slot < 0 || slot >= o->nslots) {
    set_error(std::string(who) + ": slot " + std::to_string(slot) + ": this optimiser kind has " +
              std::to_string(o->nslots) + " state slot(s)");
    return RMX_E_INVALID;
  }
  return RMX_OK;
}

}  // namespace

}  // namespace rmx

using namespace rmx;

extern "C" int rmx_optim_state_upload_rows(rmx_optim* o, int slot, int64_t id0, int64_t n, const float* weights,
                                           const float* embedding, int layout, int64_t ld, int64_t* stored) {
  const char* who = "rmx_optim_state_upload_rows";
  if (stored) *stored = 0;
  const int st = state_rows_check(who, o, slot, id0, n, weights, embedding, layout, ld);
  if (st || n == 0) return st;
  float* w = const_cast<float*>(weights);
  float* e = const_cast<float*>(embedding);
  return o->sh ? shard_state_rows(who, *o, slot, true, id0, n, w, e, layout, ld, nullptr, stored)
               : table_state_rows(*o, slot, true, id0, n, w, e, layout, ld, nullptr, stored);
}

extern "C" int rmx_optim_state_download_rows(rmx_optim* o, int slot, int64_t id0, int64_t n, float* weights,
                                             float* embedding, int layout, int64_t ld, uint8_t* owned, int64_t* found) {
  const char* who = "rmx_optim_state_download_rows";
  if (found) *found = 0;
  const int st = state_rows_check(who, o, slot, id0, n, weights, embedding, layout, ld);
  if (st || n == 0) return st;
  return o->sh ? shard_state_rows(who, *o, slot, false, id0, n, weights, embedding, layout, ld, owned, found)
               : table_state_rows(*o, slot, false, id0, n, weights, embedding, layout, ld, owned, found);
}

extern "C" int rmx_optim_state_upload_dense(rmx_optim* o, int slot, const float* mats, const float* bias) {
  const int st = state_dense_check("rmx_optim_state_upload_dense", o, slot);
  if (st) return st;
  rmx_model& m = *o->m;
  std::lock_guard<std::mutex> lk(m.mu);
  RMX_HIP(hipSetDevice(m.ctx->device));
  RMX_HIP(hipDeviceSynchronize());  // earlier steps, whichever stream they ran on
  if (mats && o->m_s[slot])
    RMX_HIP(hipMemcpy(o->m_s[slot], mats, sizeof(float) * m.mats_len, hipMemcpyHostToDevice));
  if (bias) RMX_HIP(hipMemcpy(o->b_s + slot, bias, sizeof(float), hipMemcpyHostToDevice));
  return RMX_OK;
}

extern "C" int rmx_optim_state_download_dense(rmx_optim* o, int slot, float* mats, float* bias) {
  const int st = state_dense_check("rmx_optim_state_download_dense", o, slot);
  if (st) return st;
  rmx_model& m = *o->m;
  std::lock_guard<std::mutex> lk(m.mu);
  RMX_HIP(hipSetDevice(m.ctx->device));
  RMX_HIP(hipDeviceSynchronize());
  if (mats && o->m_s[slot])
    RMX_HIP(hipMemcpy(mats, o->m_s[slot], sizeof(float) * m.mats_len, hipMemcpyDeviceToHost));
  if (bias) RMX_HIP(hipMemcpy(bias, o->b_s + slot, sizeof(float), hipMemcpyDeviceToHost));
  return RMX_OK;
}

extern "C" int rmx_optim_set_steps(rmx_optim* o, int64_t t) {
  if (!o || t < 0) {
    set_error(!o ? "rmx_optim_set_steps: the optimiser is NULL" : "rmx_optim_set_steps: t is negative");
    return RMX_E_INVALID;
  }
  std::lock_guard<std::mutex> lk(o->m->mu);
  o->steps = t;
  return RMX_OK;
}
