// param_io.hip -- host ranges of rows into and out of the device-resident parameters (include/rmx.h
// rmx_table_upload_rows / rmx_shard_upload_rows / rmx_optim_state_upload_rows and their downloads).
//
// One engine for every destination: a host id range [id0, id0 + n) streams through bounded staging (RowIo: two
// pinned host chunks, two device chunks of "io_chunk_rows" rows, whatever V is) and a scatter / gather kernel
// places each row where its owner keeps it: row p(id) div N of partition p(id) mod N (owner_perm.hpp; a
// replicated table is N = 1 with the identity).  The destination's row form is a compile-time argument type:
//   DenseRows<T>  [rows][es] embeddings + [rows] weights   (a table, an optimiser's state slots)
//   LineRows<T>   [rows][rs] lines [emb k | w | pad]        (a shard partition, a table's line copy)
// Upload pipeline per chunk c (buffer b = c & 1): the host copies the caller's rows into pinned chunk b (K_MAJOR:
// k strided segments, transposed later by the kernel), the copy stream moves it to device chunk b once kernel
// c - 2 has read that buffer, the context's stream runs the put kernel once the copy has landed.  So chunk
// c + 1's host copy and H2D run under chunk c's kernel.  Downloads mirror it: get kernel, D2H on the copy stream,
// host copy-out of chunk c - 1 under chunk c's kernel and copy.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "rmx_internal.hpp"
#include "rmx_models.hpp"

namespace rmx {

namespace {

typedef float v4f __attribute__((ext_vector_type(4)));

template <class T>
struct DenseRows {
  typedef T elem;
  static constexpr bool kLine = false;
  T* emb;
  T* w;
  int64_t es;
  int k;
  __device__ __forceinline__ T* erow(int64_t r) const { return emb + r * es; }
  __device__ __forceinline__ T* wptr(int64_t r) const { return w + r; }
  __device__ __forceinline__ int pad_end() const { return 0; }
};
template <class T>
struct LineRows {
  typedef T elem;
  static constexpr bool kLine = true;
  T* emb;  // the lines
  T* w;    // emb + k
  int64_t es;  // rs
  int k;
  __device__ __forceinline__ T* erow(int64_t r) const { return emb + r * es; }
  __device__ __forceinline__ T* wptr(int64_t r) const { return w + r * es; }
  __device__ __forceinline__ int pad_end() const { return (int)es; }
};

// One chunk: rows [id0, id0 + n) in the device chunk buffers (each nullable: that part is not moved).
struct ChunkArgs {
  int64_t id0;
  int n;
  int N, part;
  int kmajor;                 // emb is [k][n] (element j of row i at emb[j * n + i]) instead of [n][k]
  int nt;                     // put: non-temporal stores (knob "io_nt")
  float* emb;
  float* w;
  uint8_t* owned;             // get (nullable): 1 where the row's partition is `part`
  int mark_all;               // get: write owned[i] for every row (else only the 1s: a later partition's launch)
  unsigned long long* count;  // put (nullable): += rows stored
  OwnerPerm op;
};

constexpr int kIoThreads = 256;   // 4 waves of 64 ids
constexpr int kTileLd = 20;       // floats per id in the K_MAJOR transpose tile (16 + 4: rows stay 16-B aligned)

// local row of chunk row i in partition c.part, or -1 (not held there / past the chunk)
__device__ __forceinline__ int local_row(const ChunkArgs& c, int i) {
  if (i >= c.n) return -1;
  const int64_t p = owner_perm(c.id0 + i, c.op, false);
  return (int)(p % c.N) == c.part ? (int)(p / c.N) : -1;
}

__device__ __forceinline__ void st4(float* p, v4f v, int nt) {
  if (nt)
    __builtin_nontemporal_store(v, reinterpret_cast<v4f*>(p));
  else
    *reinterpret_cast<v4f*>(p) = v;
}

// Scatter of a chunk into the rows of one partition.  VEC (fp32, k = 16, rows 16-B aligned): a wave takes 64 ids;
// each lane runs the permutation for ONE id, then the wave walks its ids 8 at a time with 8 lanes per id and one
// 16-B access each -- lanes 0-3 the embedding, lane 4 the weight, lanes 5-7 the pad -- taking the id's row from
// the lane that computed it.  On line rows an upload of both parts stores all eight pieces: the whole 128-B line
// [emb | w | 0 pad] in one instruction, never a partial line followed by a second store to it; a weights-only or
// embedding-only upload stores only those bytes.  A K_MAJOR chunk is transposed through an LDS tile.  Otherwise
// (any k, bf16 elements): one thread per id, scalar over the row.
template <class A, bool VEC>
__global__ __launch_bounds__(kIoThreads) void shard_put_rows_kernel(A a, ChunkArgs c) {
  typedef typename A::elem T;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int base = blockIdx.x * kIoThreads + wv * 64;
  const int i = base + lane;
  const int row = local_row(c, i);
  if (c.count) {
    const int cnt = __popcll(__ballot(row >= 0));
    if (lane == 0 && cnt) atomicAdd(c.count, (unsigned long long)cnt);
  }
  if constexpr (VEC) {
    __shared__ __attribute__((aligned(16))) float tile[kIoThreads * kTileLd];
    if (c.kmajor && c.emb) {
      float* mine = tile + (wv * 64 + lane) * kTileLd;
      for (int j = 0; j < 16; ++j) mine[j] = i < c.n ? c.emb[(int64_t)j * c.n + i] : 0.f;
      __syncthreads();
    }
    const int g = lane >> 3, cc = lane & 7;
    const bool full = A::kLine && c.emb && c.w;
    int rows8[8];  // (every shuffle before the first divergent branch: all 64 lanes take part)
    for (int it = 0; it < 8; ++it) rows8[it] = __shfl(row, it * 8 + g);
    for (int it = 0; it < 8; ++it) {
      const int src = it * 8 + g;
      const int r = rows8[it];
      if (r < 0) continue;
      const int ii = base + src;
      float* dst = reinterpret_cast<float*>(a.erow(r));
      if (cc < 4) {
        if (!c.emb) continue;
        const v4f v = c.kmajor ? *reinterpret_cast<const v4f*>(tile + (wv * 64 + src) * kTileLd + cc * 4)
                               : reinterpret_cast<const v4f*>(c.emb)[(int64_t)ii * 4 + cc];
        st4(dst + cc * 4, v, c.nt);
      } else if (cc == 4) {
        if (!c.w) continue;
        const float wv_ = c.w[ii];
        if (full) {
          const v4f v = {wv_, 0.f, 0.f, 0.f};
          st4(dst + 16, v, c.nt);
        } else {
          *reinterpret_cast<float*>(a.wptr(r)) = wv_;
        }
      } else if (full) {
        const v4f z = {0.f, 0.f, 0.f, 0.f};
        st4(dst + cc * 4, z, c.nt);
      }
    }
  } else {
    if (row < 0) return;
    T* e = a.erow(row);
    if (c.emb)
      for (int j = 0; j < a.k; ++j) st1(e + j, c.kmajor ? c.emb[(int64_t)j * c.n + i] : c.emb[(int64_t)i * a.k + j]);
    if (c.w) st1(a.wptr(row), c.w[i]);
    if (A::kLine && c.emb && c.w)
      for (int j = a.k + 1; j < a.pad_end(); ++j) st1(e + j, 0.f);
  }
}

// The mirror: rows of one partition into the chunk buffers (fp32; bf16 elements widen exactly).  Rows of other
// partitions are not written.
template <class A, bool VEC>
__global__ __launch_bounds__(kIoThreads) void shard_get_rows_kernel(A a, ChunkArgs c) {
  typedef typename A::elem T;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int base = blockIdx.x * kIoThreads + wv * 64;
  const int i = base + lane;
  const int row = local_row(c, i);
  if (c.owned && i < c.n) {
    if (c.mark_all)
      c.owned[i] = row >= 0 ? 1 : 0;
    else if (row >= 0)
      c.owned[i] = 1;
  }
  if constexpr (VEC) {
    __shared__ __attribute__((aligned(16))) float tile[kIoThreads * kTileLd];
    const int g = lane >> 3, cc = lane & 7;
    int rows8[8];
    for (int it = 0; it < 8; ++it) rows8[it] = __shfl(row, it * 8 + g);
    for (int it = 0; it < 8; ++it) {
      const int src = it * 8 + g;
      const int r = rows8[it];
      if (r < 0) continue;
      const int ii = base + src;
      if (cc < 4) {
        if (!c.emb) continue;
        const v4f v = *reinterpret_cast<const v4f*>(reinterpret_cast<const float*>(a.erow(r)) + cc * 4);
        if (c.kmajor)
          *reinterpret_cast<v4f*>(tile + (wv * 64 + src) * kTileLd + cc * 4) = v;
        else
          reinterpret_cast<v4f*>(c.emb)[(int64_t)ii * 4 + cc] = v;
      } else if (cc == 4 && c.w) {
        c.w[ii] = *reinterpret_cast<const float*>(a.wptr(r));
      }
    }
    if (c.kmajor && c.emb) {
      __syncthreads();
      if (row >= 0) {
        const float* mine = tile + (wv * 64 + lane) * kTileLd;
        for (int j = 0; j < 16; ++j) c.emb[(int64_t)j * c.n + i] = mine[j];
      }
    }
  } else {
    if (row < 0) return;
    const T* e = a.erow(row);
    if (c.emb)
      for (int j = 0; j < a.k; ++j) {
        const float v = ld1(e + j);
        if (c.kmajor)
          c.emb[(int64_t)j * c.n + i] = v;
        else
          c.emb[(int64_t)i * a.k + j] = v;
      }
    if (c.w) c.w[i] = ld1(a.wptr(row));
  }
}

template <class A, bool VEC>
void launch_one(hipStream_t s, bool put, const A& a, const ChunkArgs& c) {
  const dim3 grid((unsigned)((c.n + kIoThreads - 1) / kIoThreads)), block(kIoThreads);
  if (put)
    hipLaunchKernelGGL((shard_put_rows_kernel<A, VEC>), grid, block, 0, s, a, c);
  else
    hipLaunchKernelGGL((shard_get_rows_kernel<A, VEC>), grid, block, 0, s, a, c);
}

template <class T>
void launch_typed(hipStream_t s, bool put, const RowTarget& t, int k, const ChunkArgs& c) {
  // the 16-B path: fp32 rows of 16 columns whose stride keeps them 16-B aligned (a line: the 32-float line)
  const bool vec = std::is_same<T, float>::value && k == 16 && (t.line ? t.rs == 32 : t.es % 4 == 0);
  if (t.line) {
    LineRows<T> a{(T*)t.emb, (T*)t.emb + k, t.rs, k};
    if constexpr (std::is_same<T, float>::value)
      if (vec) return launch_one<LineRows<T>, true>(s, put, a, c);
    launch_one<LineRows<T>, false>(s, put, a, c);
  } else {
    DenseRows<T> a{(T*)t.emb, (T*)t.w, t.es, k};
    if constexpr (std::is_same<T, float>::value)
      if (vec) return launch_one<DenseRows<T>, true>(s, put, a, c);
    launch_one<DenseRows<T>, false>(s, put, a, c);
  }
}

// one chunk into / out of every target; c.emb / c.w are dropped where a target holds no such part
int launch_chunk(hipStream_t s, bool put, const RowSpace& sp, const RowTarget* tg, int ntg, ChunkArgs c,
                 uint8_t* owned, unsigned long long* count) {
  bool first = true;
  for (int q = 0; q < ntg; ++q) {
    const RowTarget& t = tg[q];
    ChunkArgs cq = c;
    cq.part = t.part;
    if (!t.line && !t.emb) cq.emb = nullptr;
    if (!t.line && !t.w) cq.w = nullptr;
    if (sp.k <= 0) cq.emb = nullptr;
    cq.owned = t.primary ? owned : nullptr;
    cq.count = t.primary ? count : nullptr;
    cq.mark_all = first && t.primary ? 1 : 0;
    if (t.primary) first = false;
    if (t.dt == kBF16)
      launch_typed<bf16_t>(s, put, t, sp.k, cq);
    else
      launch_typed<float>(s, put, t, sp.k, cq);
    RMX_HIP(hipGetLastError());
  }
  return RMX_OK;
}

constexpr int kIoChunkDefault = 262144;

int io_ensure(RowIo& io, int k) {
  int64_t want = tuning_get("io_chunk_rows", kIoChunkDefault);
  want = std::min<int64_t>(std::max<int64_t>(want, 64), int64_t(1) << 24);
  if (io.cap == want && io.k == k) return RMX_OK;
  if (io.cap) RMX_HIP(hipDeviceSynchronize());
  io.release();
  const size_t ke = (size_t)std::max(k, 1);
  int st;
  for (int b = 0; b < 2; ++b) {
    if ((st = io.d_emb[b].alloc((size_t)want * ke, "row staging")) || (st = io.d_w[b].alloc((size_t)want, "row staging")) ||
        (st = io.d_own[b].alloc((size_t)want, "row staging"))) {
      io.release();
      return st;
    }
  }
  if ((st = io.d_cnt.alloc(1, "row staging"))) {
    io.release();
    return st;
  }
  // (cap stays 0 until everything is there: a failed HIP call below leaves a state that release() undoes)
  for (int b = 0; b < 2; ++b) {
    RMX_HIP(hipHostMalloc((void**)&io.h_emb[b], sizeof(float) * want * ke));
    RMX_HIP(hipHostMalloc((void**)&io.h_w[b], sizeof(float) * want));
    RMX_HIP(hipHostMalloc((void**)&io.h_own[b], (size_t)want));
    RMX_HIP(hipEventCreateWithFlags(&io.ev_copy[b], hipEventDisableTiming));
    RMX_HIP(hipEventCreateWithFlags(&io.ev_kern[b], hipEventDisableTiming));
  }
  RMX_HIP(hipHostMalloc((void**)&io.h_cnt, sizeof(unsigned long long)));
  RMX_HIP(hipStreamCreateWithFlags(&io.copy, hipStreamNonBlocking));
  io.cap = want;
  io.k = k;
  return RMX_OK;
}

}  // namespace

void RowIo::release() {
  if (copy) {
    (void)hipStreamSynchronize(copy);
    (void)hipStreamDestroy(copy);
  }
  copy = nullptr;
  for (int b = 0; b < 2; ++b) {
    d_emb[b].reset();
    d_w[b].reset();
    d_own[b].reset();
    if (h_emb[b]) (void)hipHostFree(h_emb[b]);
    if (h_w[b]) (void)hipHostFree(h_w[b]);
    if (h_own[b]) (void)hipHostFree(h_own[b]);
    if (ev_copy[b]) (void)hipEventDestroy(ev_copy[b]);
    if (ev_kern[b]) (void)hipEventDestroy(ev_kern[b]);
    h_emb[b] = h_w[b] = nullptr;
    h_own[b] = nullptr;
    ev_copy[b] = ev_kern[b] = nullptr;
  }
  d_cnt.reset();
  if (h_cnt) (void)hipHostFree(h_cnt);
  h_cnt = nullptr;
  cap = 0;
  k = 0;
}

int rows_check(const char* who, const void* handle, int64_t V, int64_t id0, int64_t n, int layout, int64_t ld) {
  const std::string w(who);
  if (!handle) {
    set_error(w + ": the handle is NULL");
    return RMX_E_INVALID;
  }
  if (n < 0) {
    set_error(w + ": n is negative (" + std::to_string(n) + ")");
    return RMX_E_INVALID;
  }
  if (layout != RMX_LAYOUT_K_MAJOR && layout != RMX_LAYOUT_ROW_MAJOR) {
    set_error(w + ": unknown layout " + std::to_string(layout));
    return RMX_E_INVALID;
  }
  if (layout == RMX_LAYOUT_K_MAJOR && ld < n) {
    set_error(w + ": ld " + std::to_string(ld) + " is less than n " + std::to_string(n) + " (K_MAJOR)");
    return RMX_E_INVALID;
  }
  if (id0 < 0 || id0 > V || n > V - id0) {
    set_error(w + ": id0 " + std::to_string(id0) + " + n " + std::to_string(n) + " leaves [0, " + std::to_string(V) +
              ")");
    return RMX_E_INDEX;
  }
  return RMX_OK;
}

namespace {
// Both streams of a streaming call are idle when it returns, whichever way: no queued copy still touches the
// pinned chunks or a kernel the device chunks after an early return.
struct Drain {
  hipStream_t copy, s;
  ~Drain() {
    (void)hipStreamSynchronize(copy);
    (void)hipStreamSynchronize(s);
  }
};
}  // namespace

int rows_upload(const RowSpace& sp, const RowTarget* tg, int ntg, int64_t id0, int64_t n, const float* weights,
                const float* embedding, int layout, int64_t ld, int64_t* stored) {
  if (stored) *stored = 0;
  if (n <= 0) return RMX_OK;
  RowIo& io = *sp.io;
  std::lock_guard<std::mutex> lk(io.mu);
  RMX_HIP(hipSetDevice(sp.ctx->device));
  RMX_HIP(hipDeviceSynchronize());  // earlier work on the rows, whichever stream it ran on
  int st = io_ensure(io, sp.k);
  if (st) return st;
  hipStream_t s = sp.ctx->stream;
  const Drain drain{io.copy, s};  // synchronous on return, on the error paths too
  const int k = sp.k;
  const bool km = layout == RMX_LAYOUT_K_MAJOR;
  if (k <= 0) embedding = nullptr;
  RMX_HIP(hipMemsetAsync(io.d_cnt, 0, sizeof(unsigned long long), s));
  const int nt = tuning_get("io_nt", 0);
  int64_t c = 0;
  for (int64_t i0 = 0; i0 < n; i0 += io.cap, ++c) {
    const int b = (int)(c & 1);
    const int64_t cn = std::min(io.cap, n - i0);
    RMX_HIP(hipEventSynchronize(io.ev_copy[b]));  // chunk c - 2 has left pinned buffer b
    if (weights) std::memcpy(io.h_w[b], weights + i0, sizeof(float) * cn);
    if (embedding) {
      if (km)
        for (int j = 0; j < k; ++j) std::memcpy(io.h_emb[b] + (size_t)j * cn, embedding + (size_t)j * ld + i0, sizeof(float) * cn);
      else
        std::memcpy(io.h_emb[b], embedding + (size_t)i0 * k, sizeof(float) * cn * k);
    }
    RMX_HIP(hipStreamWaitEvent(io.copy, io.ev_kern[b], 0));  // kernel c - 2 has read device buffer b
    if (weights) RMX_HIP(hipMemcpyAsync(io.d_w[b], io.h_w[b], sizeof(float) * cn, hipMemcpyHostToDevice, io.copy));
    if (embedding)
      RMX_HIP(hipMemcpyAsync(io.d_emb[b], io.h_emb[b], sizeof(float) * cn * k, hipMemcpyHostToDevice, io.copy));
    RMX_HIP(hipEventRecord(io.ev_copy[b], io.copy));
    RMX_HIP(hipStreamWaitEvent(s, io.ev_copy[b], 0));
    ChunkArgs ca{};
    ca.id0 = id0 + i0;
    ca.n = (int)cn;
    ca.N = sp.N;
    ca.kmajor = km ? 1 : 0;
    ca.nt = nt;
    ca.emb = embedding ? io.d_emb[b].get() : nullptr;
    ca.w = weights ? io.d_w[b].get() : nullptr;
    ca.op = sp.op;
    if ((st = launch_chunk(s, true, sp, tg, ntg, ca, nullptr, io.d_cnt))) break;
    RMX_HIP(hipEventRecord(io.ev_kern[b], s));
  }
  if (!st) RMX_HIP(hipMemcpyAsync(io.h_cnt, io.d_cnt, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  RMX_HIP(hipStreamSynchronize(io.copy));
  RMX_HIP(hipStreamSynchronize(s));
  if (!st && stored) *stored = (int64_t)*io.h_cnt;
  return st;
}

namespace {
// chunk rows [i0, i0 + cn) from pinned buffer b to the caller's arrays: only the rows owned here
int64_t copy_out(const RowIo& io, int b, int64_t i0, int64_t cn, int k, bool km, int64_t ld, float* weights,
                 float* embedding, uint8_t* owned) {
  const uint8_t* own = io.h_own[b];
  int64_t found = 0;
  for (int64_t i = 0; i < cn; ++i) found += own[i];
  if (owned) std::memcpy(owned + i0, own, (size_t)cn);
  if (found == cn) {
    if (weights) std::memcpy(weights + i0, io.h_w[b], sizeof(float) * cn);
    if (embedding) {
      if (km)
        for (int j = 0; j < k; ++j) std::memcpy(embedding + (size_t)j * ld + i0, io.h_emb[b] + (size_t)j * cn, sizeof(float) * cn);
      else
        std::memcpy(embedding + (size_t)i0 * k, io.h_emb[b], sizeof(float) * cn * k);
    }
    return found;
  }
  for (int64_t i = 0; found && i < cn; ++i) {
    if (!own[i]) continue;
    if (weights) weights[i0 + i] = io.h_w[b][i];
    if (!embedding) continue;
    if (km)
      for (int j = 0; j < k; ++j) embedding[(size_t)j * ld + i0 + i] = io.h_emb[b][(size_t)j * cn + i];
    else
      std::memcpy(embedding + (size_t)(i0 + i) * k, io.h_emb[b] + (size_t)i * k, sizeof(float) * k);
  }
  return found;
}
}  // namespace

int rows_download(const RowSpace& sp, const RowTarget* tg, int ntg, int64_t id0, int64_t n, float* weights,
                  float* embedding, int layout, int64_t ld, uint8_t* owned, int64_t* found) {
  if (found) *found = 0;
  if (n <= 0) return RMX_OK;
  RowIo& io = *sp.io;
  std::lock_guard<std::mutex> lk(io.mu);
  RMX_HIP(hipSetDevice(sp.ctx->device));
  RMX_HIP(hipDeviceSynchronize());
  int st = io_ensure(io, sp.k);
  if (st) return st;
  hipStream_t s = sp.ctx->stream;
  const Drain drain{io.copy, s};  // synchronous on return, on the error paths too
  const int k = sp.k;
  const bool km = layout == RMX_LAYOUT_K_MAJOR;
  if (k <= 0) embedding = nullptr;
  const int64_t nch = (n + io.cap - 1) / io.cap;
  int64_t tot = 0;
  for (int64_t c = 0; c <= nch && !st; ++c) {
    if (c < nch) {
      const int b = (int)(c & 1);
      const int64_t i0 = c * io.cap, cn = std::min(io.cap, n - i0);
      RMX_HIP(hipStreamWaitEvent(s, io.ev_copy[b], 0));  // chunk c - 2 has left device buffer b
      ChunkArgs ca{};
      ca.id0 = id0 + i0;
      ca.n = (int)cn;
      ca.N = sp.N;
      ca.kmajor = km ? 1 : 0;
      ca.emb = embedding ? io.d_emb[b].get() : nullptr;
      ca.w = weights ? io.d_w[b].get() : nullptr;
      ca.op = sp.op;
      if ((st = launch_chunk(s, false, sp, tg, ntg, ca, io.d_own[b], nullptr))) break;
      RMX_HIP(hipEventRecord(io.ev_kern[b], s));
      RMX_HIP(hipStreamWaitEvent(io.copy, io.ev_kern[b], 0));
      if (weights) RMX_HIP(hipMemcpyAsync(io.h_w[b], io.d_w[b], sizeof(float) * cn, hipMemcpyDeviceToHost, io.copy));
      if (embedding)
        RMX_HIP(hipMemcpyAsync(io.h_emb[b], io.d_emb[b], sizeof(float) * cn * k, hipMemcpyDeviceToHost, io.copy));
      RMX_HIP(hipMemcpyAsync(io.h_own[b], io.d_own[b], (size_t)cn, hipMemcpyDeviceToHost, io.copy));
      RMX_HIP(hipEventRecord(io.ev_copy[b], io.copy));
    }
    if (c >= 1) {  // the previous chunk, under this one's kernel and copy
      const int pb = (int)((c - 1) & 1);
      const int64_t i0 = (c - 1) * io.cap, cn = std::min(io.cap, n - i0);
      RMX_HIP(hipEventSynchronize(io.ev_copy[pb]));
      tot += copy_out(io, pb, i0, cn, k, km, ld, weights, embedding, owned);
    }
  }
  RMX_HIP(hipStreamSynchronize(io.copy));
  RMX_HIP(hipStreamSynchronize(s));
  if (!st && found) *found = tot;
  return st;
}

// Test / bench hook: the get and the put kernel alone on a device-resident chunk.  Rows [id0, id0 + n) (n at most
// one chunk) are gathered into device chunk 0 once, then `iters` gets and `iters` puts of that same chunk are
// timed by events on the context's stream: the puts store the values the rows already hold, so nothing changes.
int rows_kernel_ms(const RowSpace& sp, const RowTarget* tg, int ntg, int64_t id0, int64_t n, int iters, int kmajor,
                   float* get_ms, float* put_ms) {
  RowIo& io = *sp.io;
  std::lock_guard<std::mutex> lk(io.mu);
  RMX_HIP(hipSetDevice(sp.ctx->device));
  RMX_HIP(hipDeviceSynchronize());
  int st = io_ensure(io, sp.k);
  if (st) return st;
  if (n > io.cap) {
    set_error("row kernel timing: n " + std::to_string(n) + " exceeds io_chunk_rows " + std::to_string(io.cap));
    return RMX_E_INVALID;
  }
  hipStream_t s = sp.ctx->stream;
  const Drain drain{io.copy, s};
  ChunkArgs ca{};
  ca.id0 = id0;
  ca.n = (int)n;
  ca.N = sp.N;
  ca.kmajor = kmajor ? 1 : 0;
  ca.nt = tuning_get("io_nt", 0);
  ca.emb = sp.k > 0 ? io.d_emb[0].get() : nullptr;
  ca.w = io.d_w[0].get();
  ca.op = sp.op;
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  for (auto& e : ev) RMX_HIP(hipEventCreate(&e));
  st = launch_chunk(s, false, sp, tg, ntg, ca, io.d_own[0], nullptr);
  if (!st) RMX_HIP(hipEventRecord(ev[0], s));
  for (int i = 0; i < iters && !st; ++i) st = launch_chunk(s, false, sp, tg, ntg, ca, io.d_own[0], nullptr);
  if (!st) RMX_HIP(hipEventRecord(ev[1], s));
  for (int i = 0; i < iters && !st; ++i) st = launch_chunk(s, true, sp, tg, ntg, ca, nullptr, nullptr);
  if (!st) RMX_HIP(hipEventRecord(ev[2], s));
  if (!st) {
    RMX_HIP(hipEventSynchronize(ev[2]));
    float a = 0.f, b = 0.f;
    RMX_HIP(hipEventElapsedTime(&a, ev[0], ev[1]));
    RMX_HIP(hipEventElapsedTime(&b, ev[1], ev[2]));
    if (get_ms) *get_ms = a / iters;
    if (put_ms) *put_ms = b / iters;
  }
  for (auto& e : ev) (void)hipEventDestroy(e);
  return st;
}

}  // namespace rmx
