// rmx_models.hpp -- model / table / context objects behind the C ABI.
#pragma once

#include <hip/hip_runtime.h>

#include <mutex>
#include <string>
#include <vector>

#include "owner_perm.hpp"
#include "rmx_internal.hpp"

struct rmx_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
};

namespace rmx {

// Staging of the row upload / download calls (param_io.hip) of one table or shard: two pinned host chunks and
// two device chunks of `cap` rows (knob "io_chunk_rows"), a copy stream beside the context's, and per buffer
// the events "its copy is done" / "its kernel is done".  Sized by cap and k only, never by V; allocated at the
// first call, reused by later ones, freed with the owner.
struct RowIo {
  std::mutex mu;                 // one streaming call at a time
  int64_t cap = 0;
  int k = 0;
  DevBuf<float> d_emb[2];        // [cap][k] (ROW_MAJOR) or [k][rows of the chunk] (K_MAJOR)
  DevBuf<float> d_w[2];          // [cap]
  DevBuf<uint8_t> d_own[2];      // [cap] 1: the row's owner partition is held here
  DevBuf<unsigned long long> d_cnt;  // [1] rows an upload stored
  float* h_emb[2] = {nullptr, nullptr};  // pinned mirrors
  float* h_w[2] = {nullptr, nullptr};
  uint8_t* h_own[2] = {nullptr, nullptr};
  unsigned long long* h_cnt = nullptr;
  hipStream_t copy = nullptr;
  hipEvent_t ev_copy[2] = {nullptr, nullptr}, ev_kern[2] = {nullptr, nullptr};
  void release();                // after the owner's device synchronise
  ~RowIo() { release(); }
};

// Where the rows of one partition (or of the whole replicated table: N = 1, part 0) live on the device.
struct RowTarget {
  void* emb = nullptr;   // dense: row r at emb + r * es elements (null: no such part); line: row r at emb + r * rs
  void* w = nullptr;     // dense: w + r (null: no such part); line rows keep w at column k
  int64_t es = 0;
  int dt = kF32;         // element type (kF32 / kBF16)
  bool line = false;     // [emb k | w | pad] line rows of stride rs (a shard partition, a table's line copy)
  int rs = 0;
  int part = 0;          // the partition held: rows with p(id) mod N == part, at local row p(id) div N
  bool primary = true;   // counts towards stored / owned (false: a second copy of the same rows)
};
struct RowSpace {
  rmx_ctx* ctx = nullptr;
  RowIo* io = nullptr;
  OwnerPerm op;
  int N = 1;
  int k = 0;
};
// The argument checks shared by every row call (all before any device call): handle, n, layout, ld, range.
int rows_check(const char* who, const void* handle, int64_t V, int64_t id0, int64_t n, int layout, int64_t ld);
// Stream host rows [id0, id0 + n) into / out of the targets, chunk by chunk; synchronous on return.
int rows_upload(const RowSpace& sp, const RowTarget* tg, int ntg, int64_t id0, int64_t n, const float* weights,
                const float* embedding, int layout, int64_t ld, int64_t* stored);
int rows_download(const RowSpace& sp, const RowTarget* tg, int ntg, int64_t id0, int64_t n, float* weights,
                  float* embedding, int layout, int64_t ld, uint8_t* owned, int64_t* found);
// ms per launch of the get and of the put kernel alone over rows [id0, id0 + n) held in a device chunk
int rows_kernel_ms(const RowSpace& sp, const RowTarget* tg, int ntg, int64_t id0, int64_t n, int iters, int kmajor,
                   float* get_ms, float* put_ms);

}  // namespace rmx

struct rmx_table {
  rmx_ctx* ctx = nullptr;
  int64_t V = 0;
  int k = 0;
  int dtype = 0;          // RMX_DTYPE_F32 / RMX_DTYPE_BF16 (elements of w and emb)
  rmx::DevBuf<void> w;    // [V]     first-order weights (Angel "weights" row 0)
  rmx::DevBuf<void> emb;  // [V][k]  embeddings, row-major (Angel "embedding" rows 0..k-1, transposed)
  // k = 16 tables with knob "table_lines" 1 (default 0): a [V][32] line copy (elements of dtype), row =
  // [emb 16 | w | pad 15] -- one 128-B memory line per id instead of a 64-B row line plus a separate weight
  // line (fp32), or one 64-B half line instead of a 32-B row line plus a weight line (bf16, round 5).
  // Rebuilt from emb / w by every upload / fill (rmx_table_refresh_lines after writes through
  // device_ptrs); read by the models whose every table access takes a row stride
  // (rmx::model_reads_lines).  Measured ~1 % SLOWER for DeepFM layer 1 at V = 1M (0.1851 vs 0.1829 ms,
  // two A/B pairs on one box): the weight lines it saves hit the Infinity Cache, so it is off.
  rmx::DevBuf<float> line;  // (bf16 tables: bf16 elements, half as many floats)
  mutable rmx::RowIo io;    // staging of rmx_table_upload_rows / _download_rows and of its optimiser's state calls
};

namespace rmx {

struct TrainState;  // train.hip: backward workspace + rocBLAS handle

// One forward's inputs, already on the device.
struct FwdInputs {
  int B = 0;
  const int32_t* ids = nullptr;    // [B][F] or nullptr: implicit id = b*F + f (L-A path)
  const void* table = nullptr;     // [rows][k]  (elements of dtype)
  const void* wtab = nullptr;      // [rows]
  int dtype = 0;                   // kF32 / kBF16
  // row stride of `table` and stride of `wtab` in elements (0: k and 1).  ld = wld = 32 with
  // wtab = table + 16: [emb 16 | w | pad] line rows (a sharded partition read in place at one rank,
  // or a replicated table's line copy); only the models of rmx::model_reads_lines (model_forward checks)
  int ld = 0, wld = 0;
  const float* y1 = nullptr;       // precomputed first order (L-A irregular index) or nullptr
  float beta = 0.f;
  float* out = nullptr;            // [B]
};

// DCN cross stack scalars for the fused closed form (k_interact.hip cross_finish_kernel)
constexpr int kMaxFusedCross = 8;
struct CrossScalars {
  float wsum[kMaxFusedCross];  // sum_d w_l[d]
  float beta[kMaxFusedCross];  // beta_l
  float wo_sum;                // sum_d W_out[d], d < D
};

// CIN layer (xDeepFM): C_l (H x F*Hp) packed [Hp_pad/16][F][Npad][16], bias, output slice.
struct CinLayer {
  int Hp = 0, Hp_pad = 0, H = 0, Npad = 0;
  int64_t w_off = -1, b_off = -1, wo_off = -1;
  DevBuf<float> W;
  DevBuf<float> b;
  DevBuf<float> wo;     // [Npad] slice of the output Linear for this layer's pooled maps
  DevBuf<bf16_t> W3;     // kPrecS3 planes of W (k_gemm_s3.hip), in the chunk-map K order when map_on
  // kPrecS3 K-chunk map (k_gemm.hpp cin_chunk): one entry f0 | hc << 16 | pair << 30 per 16-wide
  // chunk.  Layer 1 keeps only the h <= f half of its symmetric z = x0 (x) x0 (folded weights
  // C[f,h] + C[h,f]), and an h-chunk with <= 8 live maps carries two fields per chunk.
  DevBuf<int> cmap;
  DevBuf<float> Wm;     // fp32 [ncm][Npad][16] mapped weights (the split planes' source)
  int ncm = 0, tri = 0;
  int map_on = 0;       // W3 was packed in the mapped order (knob "cin_map" at set_mats)
  // backward dL/dz = gpre C_l on the split GEMM: C_l^T packed [KTpad/16][NTpad][16] (K = H, N = F Hp)
  DevBuf<float> WT;
  DevBuf<bf16_t> WT3;
  int KTpad = 0, NTpad = 0;
  // bf16 CIN (rmx_model_set_cin_precision, k_cin_bf16.hip): C_l rounded to bf16, [steps][Npad][32] in the
  // unfolded K order; the model then holds no W / W3 / Wm / WT / WT3 for the layer
  DevBuf<bf16_t> W16;
};

}  // namespace rmx

struct rmx_model {
  std::vector<rmx::Scratch> scratch;  // see "workspace" below; first, so that it is destroyed last
  rmx_ctx* ctx = nullptr;
  int type = 0;
  int64_t input_dim = 0;
  int F = 0, k = 0;
  std::vector<int> fc, cin;
  int cross_depth = 0;
  std::vector<int32_t> sizes;  // getMatsSize
  int64_t mats_len = 0;

  // ---- device parameters (packed from mats) ----
  rmx::DevBuf<float> mats_dev;              // raw mats copy
  std::vector<rmx::DenseLayer> layers;      // tower; the last one runs the output head
  int64_t wo_off = -1, bo_off = -1;         // output Linear weights / bias in mats
  rmx::DevBuf<float> wo;                    // device [Npad of last layer]
  float bo = 0.f;
  bool has_bo = false;
  std::vector<rmx::CinLayer> cin_layers;    // xDeepFM
  int64_t wo_cin_off = -1;                  // start of the pooled-CIN slice of W_out
  int64_t cross_w_off = -1, cross_b_off = -1, wo_x_off = -1;  // DCN
  rmx::DevBuf<float> cross_w;               // [L][D]
  rmx::DevBuf<float> cross_b;               // [L]
  rmx::DevBuf<float> wo_x;                  // [D] slice of W_out for x_L
  bool dcn_fused = false;                   // cross dots fused into tower layer 1 (fcDims >= 2)
  rmx::CrossScalars cross_scalars{};
  rmx::DevBuf<int32_t> pairs;               // PNN (row, col) pairs [P][2]
  int precision = 0;                        // kF32 / kBF16 (rmx_model_set_precision)
  int cin_precision = 0;                    // kF32 / kBF16 (rmx_model_set_cin_precision; xDeepFM)
  bool params_ready = false;
  float beta = 0.f;
  bool beta_set = false;

  // ---- workspace (grown on demand) ----
  // every floating-point scratch buffer below, of the L-A staging and of TrainState, with its allocated size:
  // the ScratchBuf members, listed here while they are allocated.  What rmx_debug_poison_workspace fills.
  // (Declared in the struct's first lines, before every buffer: it outlives them all.)
  struct Workspace {                  // the batch-sized inference buffers: one capacity, dropped together
    int B = 0;
    rmx::ScratchBuf<float> h[2];      // [B][Npad] tower activations
    rmx::ScratchBuf<float> y12;       // [B] first order (+ FM)
    rmx::ScratchBuf<float> pre2;      // [B] model-specific additive term (CIN / cross)
    rmx::ScratchBuf<float> xcol;      // [B][L + 1] raw fused cross dots (DCN)
    rmx::ScratchBuf<float> ubuf[2];   // [B*k][Npad] CIN maps
    rmx::ScratchBuf<float> rowdot;    // [B*k] CIN per-row output partials
    rmx::ScratchBuf<float> opart;     // [slices][B] partial logits of a column-sliced output layer
  } ws;
  int xbuf_B = 0;                     // xbuf's own capacity (rows): grown where a path that needs it is chosen
  rmx::ScratchBuf<float> xbuf;        // [xbuf_B][Kpad0] materialised A (PNN [x | ip], generic k, DeepFM column-split x)
  // L-A staging
  int64_t la_nnz = 0;
  int la_B = 0;
  rmx::ScratchBuf<float> la_E;
  rmx::ScratchBuf<float> la_w;
  rmx::DevBuf<int64_t> la_rowptr;     // (row pointers: never in the scratch list, a leftover there would be an address)
  rmx::ScratchBuf<float> la_out;
  rmx::ScratchBuf<rmx::bf16_t> la_E16;           // bf16 models: the rounded L-A arrays
  rmx::ScratchBuf<rmx::bf16_t> la_w16;
  int64_t la16_cap = 0;
  std::vector<int64_t> h_rowptr;
  std::vector<float> h_wperm;

  rmx::TrainState* train = nullptr;          // backward (train.hip), created on first use
  struct LaGrad {                            // L-A backward staging (rmx_backward), grown on demand
    int64_t nnz = 0, B = 0, ml = 0;
    rmx::DevBuf<float> gw, ge, gm, gb, tg;
    rmx::DevBuf<int32_t> idx;
  } la_grad;

  // ---- reentrancy (rmx.h "Threading"): one caller at a time; calls on different streams are
  //      ordered on the device by an event (rmx::ModelUse) ----
  std::mutex mu;
  hipStream_t ws_stream = nullptr;  // stream of the last call that used the workspace
  hipEvent_t ws_fence = nullptr;    // recorded on it at the end of that call (or, lazy, at the hand-over)
  bool ws_fence_lazy = false;       // the fence is not recorded yet: record it on ws_stream at the hand-over

  // ---- stage timing ----
  bool timing = false;
  int timed_calls = 0;
  std::vector<std::string> stage_names;
  std::vector<float> stage_ms;
  struct Pending { int stage; hipEvent_t a, b; };
  std::vector<Pending> pending;
  std::vector<hipEvent_t> ev_pool;
};

// Device-resident optimiser of one (model, table) pair (optim.hip): the state slots, the grouping scratch of
// the sparse update and the gradient buffers of rmx_train_step_ids.  Used under its model's lock.
// Or of a (model, shard) pair (rmx_optim_create_sharded; the push, shard.hip): t is null then, and the table
// state slots hold one [rows][k] / [rows] block per partition held here (a loopback shard: nparts = N), used
// under the shard's lock, then the model's.
struct rmx_optim {
  rmx_model* m = nullptr;
  rmx_table* t = nullptr;
  rmx_shard* sh = nullptr;
  int k = 0;                       // columns of the table / shard
  int64_t rows = 0;                // rows a state block covers: the table's V, a partition's rows_per
  int nparts = 1;
  int kind = 0;
  double eta = 0, a = 0, b = 0, eps = 0;  // a: momentum / factor / beta; b: gamma (Adam)
  int64_t steps = 0;
  int nslots = 0;                  // state slots per parameter: SGD 0, Momentum / Adagrad 1, Adam 2
  bool upd_w = false, upd_e = false;  // first order (not DNN) / embeddings (not LR)
  rmx::DevBuf<float> w_s[2];            // [V]      per slot
  rmx::DevBuf<float> e_s[2];            // [V][k]   per slot
  rmx::DevBuf<float> m_s[2];            // [mats_len] per slot
  rmx::DevBuf<float> b_s;               // [2] bias slots
  rmx::DevBuf<float> hv;                // [rmx::kOptimHostVals] staging of the model's host-side values
  // grouping scratch, grown on demand (every word read by an apply is written by it first)
  int64_t cap_nnz = 0;
  rmx::DevBuf<uint32_t> keys[2];
  rmx::DevBuf<uint32_t> vals[2];
  rmx::DevBuf<uint32_t> hist;           // [256][tiles]
  rmx::DevBuf<uint32_t> bsum;           // sums of hist's 1,024-element blocks (the scan's first pass)
  rmx::DevBuf<float> part;              // [2 * windows][k + 1] chunk sums of lists longer than 512
  rmx::DevBuf<int32_t> long_head;       // [windows] start of the long list whose first chunk begins there
  // rmx_train_step_ids' gradients
  int64_t g_nnz = 0;
  rmx::DevBuf<float> g_b, g_w, g_e, g_m;  // g_b: [2] = {g_bias, loss}
  // the push of a sharded optimiser (shard.hip), grown on demand after a device synchronise
  int64_t cap_push = 0;                 // nonzeros the bucketing buffers hold
  rmx::DevBuf<int32_t> p_key;           // [nnz] owner of nonzero n (N: its id is outside the table)
  rmx::DevBuf<int32_t> p_loc;           // [nnz] its row there
  rmx::DevBuf<int32_t> p_rows;          // [nnz] local rows, bucketed by owner, ascending nonzero inside a bucket
  rmx::DevBuf<float> p_gw, p_ge;        // [nnz], [nnz][k] their gradient rows in that order
  rmx::DevBuf<int32_t> p_cnt;           // [2N] bucket sizes sent | received
  int64_t cap_pull = 0;                 // rows the owner-side list holds
  rmx::DevBuf<int32_t> r_rows;          // [received] the buckets of every source rank in rank order (own at `rank`)
  rmx::DevBuf<float> r_gw, r_ge;
  rmx::DevBuf<float> d_rx;              // [N][mats_len + 1] every rank's {g_mats, g_bias}
  rmx::DevBuf<float> d_sum;             // [mats_len + 1] their sum in rank order
};

namespace rmx {
constexpr int kOptimHostVals = 4 + 2 * kMaxFusedCross;  // beta, bo, wsum[L], beta_l[L], wo_sum, loss
int optim_alloc(rmx_optim& o);    // state slots (zero) after the argument checks
void optim_release(rmx_optim& o);
// One step from per-nonzero gradients (each nullable), the model's lock held by the caller.  Synchronises the
// stream when the model keeps a value on the host that the step changed (the global bias; bo; DCN's
// cross_scalars) or when sync is set; *loss (host, nullable) then receives loss_dev[0].
int optim_apply(rmx_optim& o, hipStream_t s, int32_t B, const int32_t* ids, const float* g_bias, const float* g_w,
                const float* g_emb, const float* g_mats, const float* loss_dev, float* loss, bool sync);
int optim_ensure_grads(rmx_optim& o, int64_t nnz);  // rmx_train_step_ids' gradient buffers for nnz nonzeros
// The two halves of optim_apply, for the sharded push (shard.hip).  Both read the step count o.steps + 1; the
// dense half then counts the step.
struct SparseRows {  // the rows a sparse update writes, with their state slots
  int64_t V = 0;     // keys >= V are skipped
  int k = 0;
  float* w = nullptr;    // [V]; rs > 0: the w slot of row 0 (emb + k), stride rs
  float* emb = nullptr;  // [V][k]; rs > 0: [V][rs] line rows [emb k | w | pad] of a shard partition
  int rs = 0;
  float* line = nullptr;  // a table's line copy (rs == 0 only)
  float* ws[2] = {nullptr, nullptr};  // state, dense [V] / [V][k] either way
  float* es[2] = {nullptr, nullptr};
};
int optim_sparse_update(rmx_optim& o, hipStream_t s, int64_t nnz, const int32_t* ids, const SparseRows& t,
                        const float* g_w, const float* g_emb);
int optim_dense_update(rmx_optim& o, hipStream_t s, const float* g_bias, const float* g_mats, const float* loss_dev,
                       float* loss, bool sync);
// One stable pass over keys[0, n): the positions grouped by key, ascending inside a key, into o.vals[0] and the
// sorted keys into o.keys[0].  Keys outside [0, nkeys) count as nkeys (last); nkeys < 256.
int optim_bucket_sort(rmx_optim& o, hipStream_t s, int64_t n, const int32_t* keys, int nkeys);
// out[i] = planes[0][i] + planes[1][i] + ... in that order (fp32), planes [N][len]
int optim_sum_planes(hipStream_t s, int N, int64_t len, const float* planes, float* out);
// the argument checks and hyper-parameters shared by rmx_optim_create / rmx_optim_create_sharded (capi.hip): a new
// optimiser for model m without its table or shard, or a status
int optim_new(const char* who, rmx_model* m, int kind, const double* hyper, int n_hyper, rmx_optim** out);
// the collective apply of a sharded optimiser (shard.hip; takes the shard's lock, then the model's)
int shard_optim_apply(rmx_optim& o, hipStream_t s, int32_t B, const int32_t* ids, const float* g_bias,
                      const float* g_w, const float* g_emb, const float* g_mats);
int model_build(rmx_model& m);
void model_init_mats(const rmx_model& m, uint64_t seed, float* mats);
void model_release(rmx_model& m);
int model_load_mats(rmx_model& m, const float* host_mats, bool sync);
// the packed forms rebuilt from mats_dev on stream s (no host values: bo / cross_scalars stay as they are)
int model_repack(rmx_model& m, hipStream_t s);
int model_set_precision(rmx_model& m, int dtype);
int model_set_cin_precision(rmx_model& m, int dtype);
// backward and optimisers are not defined for a bf16 CIN: RMX_E_INVALID (message set) on such a model
int cin_bf16_rejects(const char* who, const rmx_model* m);
int model_forward(rmx_model& m, hipStream_t s, const FwdInputs& in);
// models whose every table read takes a row stride (DeepFM / DNN at k = 16, LR): they can read
// [emb | w | pad] line rows in place (FwdInputs::ld / wld)
bool model_reads_lines(const rmx_model& m);
// the forward's table operands: the line copy when the table has one and the model reads lines
void table_inputs(const rmx_table& t, const rmx_model& m, FwdInputs& in);
int table_refresh_lines(rmx_table& t);
int launch_pack_lines(hipStream_t s, int64_t V, const void* emb, const void* w, void* line, int dt);
int model_forward_host(rmx_model& m, int B, int64_t nnz, const int64_t* index, bool regular, bool sorted,
                       float bias, const float* weights, const float* embedding, const float* mats,
                       float* out);
int model_collect_timing(rmx_model& m);
int model_ensure_ws(rmx_model& m, int B);  // inference workspace (y12, h, ...) for batches <= B
int model_stage_host(rmx_model& m, int B, int64_t nnz, const int64_t* index, bool regular, bool sorted,
                     float bias, const float* weights, const float* embedding, const float* mats, FwdInputs* in);

// Backward (train.hip).  One training pass over a batch: forward with stored activations, BCE
// loss, and the gradients RecModel.backward writes back (all device pointers; g_w / g_emb may be
// null).  index: device int32 COO rows of the nnz weights (null: n / F).  loss: device [1].
struct TrainOutputs {
  const float* targets = nullptr;   // [B]
  const int32_t* index = nullptr;   // [nnz] or null
  int64_t nnz = 0;
  float* g_bias = nullptr;          // [1]
  float* g_w = nullptr;             // [nnz]
  float* g_emb = nullptr;           // [nnz * k]
  float* g_mats = nullptr;          // [mats_len]
  float* loss = nullptr;            // [1]
};
int model_train(rmx_model& m, hipStream_t s, const FwdInputs& in, const TrainOutputs& o);
void train_release(rmx_model& m);

// Serialises the callers of one model (its workspace, staging buffers and timing state are shared):
// the host lock is held for the whole call, and the call's last queued work is marked by an event;
// a call on another stream than the previous one first makes its stream wait for that event, so
// the previous call's kernels are done with the workspace before this call's run.  (The event is
// recorded at the end of every call, while the caller's stream is known to be alive.)
template <class T>
struct StreamUse {
  T& o;
  hipStream_t s;
  std::unique_lock<std::mutex> lk;
  int st = RMX_OK;
  // The fence is recorded lazily (round 6, knob "lazy_fence") for calls on the object's own context stream:
  // only when a later call arrives on another stream, on that context stream, under the lock -- it then
  // follows every operation the previous call enqueued there, which is all the hand-over needs.  Recorded
  // after every call, the marker sits between each pair of back-to-back launches.  A caller's own stream
  // keeps the eager record: it may be destroyed before the next call, the context's stream cannot be (the
  // object holds its context).
  bool lazy;
  StreamUse(T& oo, hipStream_t ss)
      : o(oo), s(ss), lk(oo.mu),
        lazy(oo.ctx && ss == oo.ctx->stream && tuning_get("lazy_fence", 0) != 0) {
    if (!o.ws_fence && hipEventCreateWithFlags(&o.ws_fence, hipEventDisableTiming) != hipSuccess) {
      o.ws_fence = nullptr;
      st = RMX_E_HIP;
    } else if (o.ws_stream && o.ws_stream != s) {
      if ((o.ws_fence_lazy && hipEventRecord(o.ws_fence, o.ws_stream) != hipSuccess) ||
          hipStreamWaitEvent(s, o.ws_fence, 0) != hipSuccess)
        st = RMX_E_HIP;
    }
    if (st) set_error("stream hand-over: HIP event create / wait failed");
  }
  ~StreamUse() {
    if (!o.ws_fence) return;
    if (lazy) {
      o.ws_stream = s;
      o.ws_fence_lazy = true;
    } else if (hipEventRecord(o.ws_fence, s) == hipSuccess) {
      o.ws_stream = s;
      o.ws_fence_lazy = false;
    }
  }
};
typedef StreamUse<rmx_model> ModelUse;

// Records HIP events around a stage on stream s when the model's timing is enabled.
struct StageTimer {
  rmx_model& m;
  hipStream_t s;
  int idx = -1;
  hipEvent_t a = nullptr;
  StageTimer(rmx_model& mm, hipStream_t ss, const char* name);
  ~StageTimer();
};
int shard_create(rmx_ctx* ctx, int64_t V, int k, int N, int rank, const void* unique_id, rmx_group* group,
                 rmx_shard** out);
int shard_destroy(rmx_shard* sh);
// The state row calls of a sharded optimiser (shard.hip; takes the shard's lock, then the model's): slot's
// [rows][k] / [rows] blocks of the partitions held here as dense targets.  up: upload (else download).
int shard_state_rows(const char* who, rmx_optim& o, int slot, bool up, int64_t id0, int64_t n, float* weights,
                     float* embedding, int layout, int64_t ld, uint8_t* owned, int64_t* count);
int64_t shard_num_rows(const rmx_shard* sh);

// kernels specific to the interaction encoders
int launch_pack_cin(hipStream_t s, const float* mats, int F, CinLayer& L);
std::vector<int> cin_chunk_map(int F, int Hp, bool tri);
int launch_pack_cin_map(hipStream_t s, const float* mats, int F, CinLayer& L);
int launch_pack_cin_t(hipStream_t s, const float* mats_dev, int F, CinLayer& c);
int launch_cin_dz_s3(hipStream_t s, const CinLayer& c, int rows, const float* gpre, int ldg, float* dz, int ldz);
int64_t cin_bf16_elems(int F, int Hp, int Npad);
int launch_pack_cin_bf16(hipStream_t s, const float* mats, int F, CinLayer& L);
int launch_cin_layer_bf16(hipStream_t s, const CinLayer& L, bool first, bool last, int B, int F, int k,
                          const int32_t* ids, const float* table, const float* u_prev, float* u_out, float* rowdot,
                          int ld = 0);
int launch_cin_layer(hipStream_t s, const CinLayer& L, bool first, bool last, int B, int F, int k,
                     const int32_t* ids, const float* table, const float* u_prev, float* u_out,
                     float* rowdot, int ld = 0);
int launch_cross_finish(hipStream_t s, int B, int L, const float* xcol, const CrossScalars& cs, float* pre2);
int launch_cross(hipStream_t s, int B, int F, int k, int L, const int32_t* ids, const void* table, int dt,
                 const float* cross_w, const float* cross_b, const float* wo_x, float* pre2);
int launch_product(hipStream_t s, int B, int F, int k, const int32_t* ids, const void* table, int dt,
                   const int32_t* pairs, int P, void* xbuf, int xdt, int ldx);
// the generic product kernel's dynamic LDS: the rows [F k + 1] of a block's four samples, at most a CU's 160 KB
// (every PNN can reach it: the host-array forward passes no id array, which the k = 16 kernel needs)
constexpr int kProductMaxD = 160 * 1024 / 16 - 1;
inline size_t product_lds_bytes(int F, int k) { return sizeof(float) * 4 * ((size_t)F * k + 1); }
inline bool product_fits_lds(int F, int k) { return (int64_t)F * k <= kProductMaxD; }
int launch_gather_x(hipStream_t s, int B, int F, int k, const int32_t* ids, const void* table, int dt, void* xbuf,
                    int xdt, int ldx);
int tower_npad_for(int N);
// DeepFM's whole fp32 tower for small batches, one block per 16 samples (k_small_s3.hip)
bool tower_small_s3_usable(const rmx_model& m, int M, int F, int k, bool ids);
int launch_tower_small_s3(hipStream_t s, const rmx_model& m, int M, int F, const int32_t* ids, const float* table,
                          int ld, const float* wtab, int wld, const OutArgs& oa);
int cin_npad_for(int H);
}  // namespace rmx
