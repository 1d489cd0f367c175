/*
 * rmx.h -- C ABI of the MI355X-native CTR forward path (librmx.so).
 *
 * Drop-in boundary for the reference's model plugin API
 *   abstract class RecModel           yr/model/RecModel.scala:6-127
 * and for the Angel-PS pull + gather that feeds it
 *   ParRecModel.pull* / make*         yr/model/ParRecModel.scala:165-199, 270-306
 * (paths relative to /root/reference/src/main/scala/, yr/ = io/yaochi/recommendation/).
 *
 * Two levels, one library:
 *   L-A  rmx_forward():      the exact RecModel.forward(batchSize, batch, bias, weights,
 *                            embeddings, embeddingDim, mats, matSizes[, fields]) contract
 *                            on host buffers (RecModel.scala:37-63, buildParams :146-155).
 *   L-B  rmx_forward_ids():  device-resident table + device ids (replaces pull* + make*).
 *
 * Conventions: every entry point returns 0 (RMX_OK) or a negative RMX_E_* code and
 * sets a thread-local message readable with rmx_last_error().  Calls on one model
 * are synchronous on return for L-A; L-B calls are asynchronous on the given
 * stream (pass NULL for the model's own stream; rmx_stream_sync to wait).
 * No torch types: plain pointers and sizes only.
 */
#ifndef RMX_H
#define RMX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RMX_ABI_VERSION 1

/* Status codes -- mirror the reference's failure modes. */
#define RMX_OK 0
#define RMX_E_INVALID (-1)  /* bad argument / missing params-map key (NoSuchElementException)      */
#define RMX_E_INDEX (-2)    /* COO row index >= batchSize: bnn/Scatter.scala:29-30 require(...)       */
#define RMX_E_SHAPE (-3)    /* nnz*k != B*F*k: BigDL Reshape(B, F, k) size mismatch                    */
#define RMX_E_TYPE (-4)     /* unknown model type / array missing for the RecModelType (MatchError)    */
#define RMX_E_HIP (-5)      /* HIP runtime error                                                      */
#define RMX_E_NOMEM (-6)    /* device allocation failed                                               */
#define RMX_E_MATS (-7)     /* mats length / matSizes disagree with getMatsSize                       */
#define RMX_E_COMM (-8)     /* RCCL error in the sharded-table exchange                               */

/* Model kinds: yr/model/{lr,deepfm,xdeepfm,dcn,pnn,dnn}/ */
#define RMX_MODEL_LR 0
#define RMX_MODEL_DEEPFM 1
#define RMX_MODEL_XDEEPFM 2
#define RMX_MODEL_DCN 3
#define RMX_MODEL_PNN 4
#define RMX_MODEL_DNN 5

/* RecModelType (yr/model/RecModelType.scala:5-8). */
#define RMX_BIAS_WEIGHT 0
#define RMX_BIAS_WEIGHT_EMBEDDING 1
#define RMX_BIAS_WEIGHT_EMBEDDING_MATS 2
#define RMX_BIAS_WEIGHT_EMBEDDING_MATS_FIELD 3

/* Element types of tables and model parameters. */
#define RMX_DTYPE_F32 0
#define RMX_DTYPE_BF16 1

/* Embedding-table host layouts for rmx_table_upload. */
#define RMX_LAYOUT_K_MAJOR 0   /* reference Angel PS layout: k rows x V columns (ParRecModel.scala:95-101) */
#define RMX_LAYOUT_ROW_MAJOR 1 /* V rows x k columns                                                      */

#define RMX_FORMAT_LIBSVM 0    /* "label id:value ..."          SampleParser.parseLIBSVM (SampleParser.scala:23-51) */
#define RMX_FORMAT_LIBFFM 1    /* "label field:id:value ..."    SampleParser.parseLIBFFM (SampleParser.scala:53-85) */

typedef struct rmx_ctx rmx_ctx;
typedef struct rmx_model rmx_model;
typedef struct rmx_table rmx_table;
typedef struct rmx_shard rmx_shard;
typedef struct rmx_group rmx_group;
typedef struct rmx_samples rmx_samples;

/* ------------------------------------------------------------------ misc -- */
const char* rmx_last_error(void);
int rmx_abi_version(void);

/* Process-wide tuning knobs (kernel variant selection for A/B timing in one process).
 * Known keys (README.md lists them): "f32_split", "s3_tower", "s3_dense", "s3_cin", "tower_variant" (GEMM
 * engine and tile variants, csrc/k_gemm.hpp, k_gemm_s3.hip), "fm_fuse", "fm_y1", "fo_fuse" (first
 * order / FM inside tower layer 1), "wgrad_s3" (training dW kernel, csrc/train.hip).  Unknown keys
 * are stored and ignored.  rmx_get_tuning returns def when the key was never set; setting
 * RMX_TUNING_DEFAULT removes the key (back to the built-in default). */
#define RMX_TUNING_DEFAULT (-2147483647 - 1)
int rmx_set_tuning(const char* key, int value);
int rmx_get_tuning(const char* key, int def);

/* ------------------------------------------------------------- context ---- */
/* One context per (process, GPU).  Owns a HIP stream. */
int rmx_ctx_create(int device, rmx_ctx** out);
int rmx_ctx_destroy(rmx_ctx* ctx);
void* rmx_ctx_stream(rmx_ctx* ctx);            /* hipStream_t of the context */
int rmx_stream_sync(void* stream);             /* hipStreamSynchronize        */

/* Device memory helpers for L-B callers (ids / outputs resident in HBM). */
int rmx_malloc(rmx_ctx* ctx, size_t bytes, void** dptr);
int rmx_free(rmx_ctx* ctx, void* dptr);
int rmx_memcpy_htod(rmx_ctx* ctx, void* dst, const void* src, size_t bytes);
int rmx_memcpy_dtoh(rmx_ctx* ctx, void* dst, const void* src, size_t bytes);

/* HIP events on the given stream (NULL = context stream), for in-band timing. */
int rmx_event_create(void** ev);
int rmx_event_destroy(void* ev);
int rmx_event_record(void* ev, void* stream);
int rmx_event_elapsed_ms(void* start, void* stop, float* ms);

/* ---------------------------------------------------------------- model ---- */
/* new LR(inputDim)                                       yr/model/lr/LR.scala:10
 * new DeepFM(inputDim, nFields, embeddingDim, fcDims)      yr/model/deepfm/DeepFM.scala:10
 * new XDeepFM(inputDim, nFields, embeddingDim, fcDims, cinDims)  yr/model/xdeepfm/XDeepFM.scala:10
 * new DCN(inputDim, nFields, embeddingDim, crossDepth, fcDims)   yr/model/dcn/DCN.scala:10
 * new PNN(inputDim, nFields, embeddingDim, fcDims)         yr/model/pnn/PNN.scala:10
 * new DNN(inputDim, nFields, embeddingDim, fcDims)         yr/model/dnn/DNN.scala:10
 * Unused arguments are ignored (pass 0 / NULL).  ctx may be NULL for a host-only model that
 * answers the metadata calls (getMatsSize ...) without a GPU. */
int rmx_model_create(rmx_ctx* ctx, int type, int64_t input_dim, int n_fields, int embedding_dim,
                     const int32_t* fc_dims, int n_fc, const int32_t* cin_dims, int n_cin,
                     int cross_depth, rmx_model** out);
int rmx_model_destroy(rmx_model* m);
/* RecModel.getType / getMatsSize / getInputDim / getEmbeddingDim (RecModel.scala:7, :121-125).
 * getMatsSize writes up to cap ints into sizes and stores the full count in *n. */
int rmx_model_get_type(const rmx_model* m);
int rmx_model_get_mats_size(const rmx_model* m, int32_t* sizes, int cap, int* n);
int64_t rmx_model_mats_len(const rmx_model* m);
int64_t rmx_model_get_input_dim(const rmx_model* m);
int rmx_model_get_embedding_dim(const rmx_model* m);

/* L-A: RecModel.forward(batchSize, batch: CooLongFloatMatrix, bias, weights, embeddings,
 *        embeddingDim, mats, matSizes[, fields]): Array[Float]     RecModel.scala:9-63
 * index[nnz] = batch.getRowIndices, feats[nnz] = batch.getColIndices (unused by the math,
 * as in the reference), weights[nnz] / embedding[nnz*k] already gathered by the caller,
 * bias[1].  Arrays not used by the model's RecModelType may be NULL.  fields is ignored
 * (no reference model reads it).  out[batch_size] receives sigmoid probabilities. */
int rmx_forward(rmx_model* m, int32_t batch_size, int64_t nnz, const int64_t* index,
                const int64_t* feats, const float* bias, const float* weights,
                const float* embedding, int32_t embedding_dim, const float* mats,
                const int32_t* mat_sizes, int32_t n_sizes, const int64_t* fields, float* out);

/* L-A backward: RecModel.backward(batchSize, batch, bias, weights, embeddings, embeddingDim,
 *        mats, matSizes[, fields], targets): Float                RecModel.scala:65-115
 * Same arrays and checks as rmx_forward plus targets[batch_size] (label > 0 -> 1).  On return the
 * caller's bias / weights / embedding / mats arrays hold the GRADIENTS, as the reference writes
 * them back in place (yr/util/GradUtil.scala:7-42, BackwardUtil.scala:6-30), and *loss the mean
 * BCE loss (BigDL BCECriterion, sizeAverage).  fp32 models; every model kind (LR, DeepFM, xDeepFM,
 * DCN, PNN, DNN). */
int rmx_backward(rmx_model* m, int32_t batch_size, int64_t nnz, const int64_t* index,
                 const int64_t* feats, float* bias, float* weights, float* embedding,
                 int32_t embedding_dim, float* mats, const int32_t* mat_sizes, int32_t n_sizes,
                 const int64_t* fields, const float* targets, float* loss);

/* Deterministic synthetic mats (Xavier-uniform weights, U(-0.01, 0.01) biases), bit-identical
 * to oracle/orc_init_mats; works on host-only models (ctx == NULL). */
int rmx_model_init_mats(const rmx_model* m, uint64_t seed, float* mats);

/* L-B parameters: load mats (getMatsSize layout) and the global bias once, on device. */
int rmx_model_set_mats(rmx_model* m, const float* mats, int64_t n_mats);
int rmx_model_set_bias(rmx_model* m, float bias);
/* RMX_DTYPE_BF16: Linear weights stored bf16 (rounded to nearest even when mats are loaded), the
 * towers on bf16 MFMA with fp32 accumulation, stored activations bf16 (BASELINE.json configs[4]).
 * Biases, the output Linear and DCN cross vectors stay fp32.  Call before rmx_model_set_mats.
 * L-B needs a table of the same dtype; L-A rounds the caller's fp32 arrays.  Not for xDeepFM (its
 * CIN alone takes bf16 operands: rmx_model_set_cin_precision). */
int rmx_model_set_precision(rmx_model* m, int dtype);
/* xDeepFM only.  RMX_DTYPE_BF16: the CIN layers run on bf16 MFMA with fp32 accumulation.  The table, the
 * DNN tower, the first order, the pooled sums, the output Linear and every stored activation stay fp32
 * (the model's precision stays RMX_DTYPE_F32: it still takes an fp32 table or shard).
 * Two values are stored bf16, each rounded once to nearest even: the CIN weights C_l, element by element
 * as given in mats, when the mats are loaded (rmx_model_get_mats still returns the caller's fp32 values);
 * and the generated operand z[f * H_prev + h] = bf16(fl32(x0[f] * u_prev[h])).  Accumulation, CIN biases,
 * ReLU, the maps u_l kept between layers, the sum-pool and the CIN slice of the output Linear are fp32.
 * Call before rmx_model_set_mats (it drops the loaded parameters); setting the current value does nothing.
 * RMX_E_INVALID for a NULL or host-only model, a model that is not an xDeepFM, or another dtype.
 * Forward only: on a bf16-CIN model rmx_backward, rmx_backward_ids, rmx_backward_pulled, rmx_optim_create,
 * rmx_optim_create_sharded, rmx_train_step_ids and rmx_train_step_sharded fail with RMX_E_INVALID. */
int rmx_model_set_cin_precision(rmx_model* m, int dtype);
int rmx_model_get_cin_precision(const rmx_model* m);   /* RMX_DTYPE_F32 (default) / RMX_DTYPE_BF16; <0 on NULL */

/* ---------------------------------------------------------------- table ---- */
/* HBM-resident first-order weights + embedding table (replaces the Angel PS rows
 * "weights" and "embedding", ParRecModel.scala:74-105).  Stored row-major [V][k]. */
int rmx_table_create(rmx_ctx* ctx, int64_t num_rows, int embedding_dim, rmx_table** out);
/* dtype RMX_DTYPE_BF16: the table stores bf16 (BASELINE.json configs[4]); uploads and the
 * synthetic fill round fp32 values to nearest even. */
int rmx_table_create_ex(rmx_ctx* ctx, int64_t num_rows, int embedding_dim, int dtype, rmx_table** out);
int rmx_table_dtype(const rmx_table* t);
int rmx_table_destroy(rmx_table* t);
/* Host upload; weights may be NULL, embedding may be NULL (then left as is). */
int rmx_table_upload(rmx_table* t, const float* weights, const float* embedding, int layout);
/* Deterministic synthetic fill, bit-identical to oracle/orc_gen_table (U(-0.05, 0.05)). */
int rmx_table_fill_synthetic(rmx_table* t, uint64_t seed);
int64_t rmx_table_rows(const rmx_table* t);
int rmx_table_embedding_dim(const rmx_table* t);  /* k of the table (-1: NULL) */
/* With knob "table_lines" 1 (default 0), fp32 k = 16 tables also hold a [rows][32] line copy
 * ([emb 16 | w | pad]: one 128-B memory line per id) that DeepFM / DNN / LR forwards read; every
 * upload / fill rebuilds it.  After writing the table through rmx_table_device_ptrs, call
 * rmx_table_refresh_lines (it also builds or drops the copy after the knob changes). */
int rmx_table_refresh_lines(rmx_table* t);
/* Device pointers of the table (for debugging/parity only; elements of the table's dtype). */
int rmx_table_device_ptrs(const rmx_table* t, void** d_weights, void** d_embedding);

/* Synthetic field-partitioned ids into device memory, bit-identical to orc_gen_ids. */
int rmx_gen_ids(rmx_ctx* ctx, uint64_t seed, int64_t row0, int32_t batch, int32_t n_fields,
                int64_t num_rows, int32_t* d_ids, void* stream);
/* L-B backward on the device-resident table: one training pass (forward with stored
 * activations, BCE, gradients) over ids [B][F].  Device outputs, each may be NULL: g_bias[1],
 * g_weights[B*F] (per nonzero, Scatter backward), g_embedding[B*F*k] (per nonzero),
 * g_mats[mats_len] (getMatsSize layout), loss[1].  The sparse per-nonzero gradients are what the
 * reference hands to makeGrad/push (ParRecModel.scala:439-478). */
int rmx_backward_ids(rmx_model* m, const rmx_table* t, int32_t batch, const int32_t* d_ids,
                     const float* d_targets, float* d_g_bias, float* d_g_weights, float* d_g_embedding,
                     float* d_g_mats, float* d_loss, void* stream);

/* ------------------------------------------------------------ optimiser ---- */
/* Device-resident optimiser step: what the reference's optimize() does after the backward
 * (ParRecModel.scala:439-478): sum the per-nonzero gradients per distinct id (makeWeightsGrad /
 * makeEmbeddingGrad, :293-328) and push them through an optimiser (pushWeightBiasEmbeddingMats, :225-253,
 * optim/Async{SGD,Momentum,Adagrad,Adam}.scala), on the table rows, mats and the global bias in place.
 * hyper[n_hyper]: the kind's hyper-parameters in the order shown; trailing ones left out take the defaults
 * shown (the reference's constructor defaults); eta has none.  All arithmetic is fp32 on the device, g the
 * aggregated gradient, t the optimiser's step count (1 on the first apply, the same for every group):
 *   SGD       p -= eta g
 *   Momentum  v = momentum v + g;  p -= eta v
 *   Adagrad   s = factor s + (1 - factor) g^2;  p -= eta g / (sqrt(s) + eps)
 *   Adam      m = beta m + (1 - beta) g;  v = gamma v + (1 - gamma) g^2;
 *             p -= eta (m / (1 - beta^t)) / (sqrt(v / (1 - gamma^t)) + eps)      (the powers: host, double)
 * No weight decay.  The reference's shared numUpdates counter, which one push bumps once per pushed group (so
 * its groups see different step counts), is deliberately NOT reproduced: Angel's server-side optimiser
 * math is not part of the reference tree, and one step count per apply is the textbook form the tests pin.
 * Sparse semantics (Angel's sparse PSF update): only rows whose id occurs in the batch change, parameters and
 * state alike; every other row keeps its bits.  State: zero-initialised slots allocated at create (SGD 0,
 * Momentum / Adagrad 1, Adam 2 per parameter): [V][k] and [V] for the table, mats_len and 1 for mats and the
 * bias; LR allocates no embedding state, DNN no first-order state.
 * Summation order (a contract): an id's gradient is the fp32 sum of its nonzeros' gradients in ascending
 * nonzero order starting from the first term (the reference's addTo loop, :316-322); a list of more than 512
 * occurrences is summed in consecutive chunks of 512 in that order, and the chunk sums are then added in chunk
 * order.  No float atomics: results are bitwise repeatable and independent of the launch geometry.  Ids outside
 * [0, V) are skipped and never addressed.
 * Sharded summation order (a contract, rmx_optim_create_sharded below): one step on a shard over ranks 0..N-1 is,
 * bit for bit, rmx_optim_apply on a replicated table given the ranks' batches concatenated in ascending rank order
 * (ids, g_weights and g_embedding concatenated) -- for the table rows and their state.  An id's gradient is the
 * fp32 sum of its occurrences in ascending (rank, nonzero) order, long lists in the same chunks of 512; ids outside
 * [0, V) are skipped and never addressed, and a partition's zero row stays zero; t is one per apply.  The mats and
 * bias gradients are the fp32 sums of the ranks' gradients, added in ascending rank order starting from rank 0's,
 * then pushed through the same elementwise update and repack: every rank computes the same bits, so the
 * replicas' mats, bias and host-side copies stay identical without a broadcast.  Gradients are SUMMED over the
 * ranks, not averaged (the reference applies every worker's push at full weight): a caller who wants the global
 * mean scales eta.  No float atomics here either.
 * fp32 models and fp32 tables only (RMX_E_INVALID otherwise); host-only model,
 * NULL arguments, unknown kind, a negative or non-finite eta: RMX_E_INVALID; table k != model k: RMX_E_SHAPE.
 * Every check runs before any device call. */
typedef struct rmx_optim rmx_optim;
#define RMX_OPTIM_SGD 0       /* hyper: {eta}                         AsyncSGD(eta)                 */
#define RMX_OPTIM_MOMENTUM 1  /* hyper: {eta, momentum=0.9}           AsyncMomentum                 */
#define RMX_OPTIM_ADAGRAD 2   /* hyper: {eta, factor=0.9, eps=1e-7}   AsyncAdagrad (decayed squares)*/
#define RMX_OPTIM_ADAM 3      /* hyper: {eta, gamma=0.99, beta=0.9, eps=1e-7}  AsyncAdam            */
int rmx_optim_create(rmx_model* m, rmx_table* t, int kind, const double* hyper, int n_hyper, rmx_optim** out);
int rmx_optim_destroy(rmx_optim* o);              /* before its model and table */
int64_t rmx_optim_steps(const rmx_optim* o);
/* Device pointers of state slot `slot` (0: v / s / m, 1: Adam's v), for debugging / parity only: [V], [V][k],
 * [mats_len] and [1] floats; each output nullable; NULL where the optimiser holds no such state. */
int rmx_optim_state_ptrs(const rmx_optim* o, int slot, void** d_weights, void** d_embedding, void** d_mats,
                         void** d_bias);
/* Apply one step from per-nonzero gradients in rmx_backward_ids' layout (each nullable = group untouched):
 * d_ids [batch * nFields], d_g_bias [1], d_g_weights [batch * nFields], d_g_embedding [batch * nFields * k],
 * d_g_mats [mats_len].  After the update of mats every packed form the forward and backward read is rebuilt
 * from them on the stream, and a table's line copy (knob "table_lines") gets the touched rows too.
 * Asynchronous on the stream, EXCEPT where the step changes a value the model keeps on the host, which is
 * then refreshed with one small device-to-host copy and a stream synchronise: the global bias (every model,
 * when d_g_bias is given); with d_g_mats, the output Linear's bias (DeepFM, DNN, PNN) and DCN's closed-form
 * cross scalars.  (xDeepFM and LR with d_g_bias NULL stay asynchronous.) */
int rmx_optim_apply(rmx_optim* o, int32_t batch, const int32_t* d_ids, const float* d_g_bias,
                    const float* d_g_weights, const float* d_g_embedding, const float* d_g_mats, void* stream);
/* backward into optimiser-owned buffers + apply; *loss (host, nullable) = mean BCE. Synchronous on return. */
int rmx_train_step_ids(rmx_model* m, const rmx_table* t, rmx_optim* o, int32_t batch, const int32_t* d_ids,
                       const float* d_targets, float* loss, void* stream);
int rmx_model_get_mats(rmx_model* m, float* mats, int64_t n_mats);   /* D2H of the current mats */
int rmx_model_get_bias(const rmx_model* m, float* bias);

/* Predict loop over a device-resident row set (ParRecModel.predict*, ParRecModel.scala:519-581):
 * scores[r] for rows r < n_rows of ids [n_rows][F], forwards of `batch` rows. */
int rmx_predict_ids(rmx_model* m, const rmx_table* t, int64_t n_rows, const int32_t* d_ids,
                    int32_t batch, float* d_scores, void* stream);
/* AUC of (label > 0, score) pairs on the device (the examples' per-epoch metric,
 * example/DeepFMLocalExample.scala:44-52): Mann-Whitney statistic, tied scores count 1/2.
 * *auc = NaN when one class is empty.  Synchronises the stream. */
int rmx_auc(rmx_ctx* ctx, int64_t n, const float* d_labels, const float* d_scores, double* auc,
            void* stream);

/* Zipf-like ids (SURVEY.md §8d secondary): rank r of field f drawn with P(r) ~ (r+1)^-exponent
 * (continuous power-law inversion, double precision), id = f * (num_rows / n_fields) + r. */
int rmx_gen_ids_zipf(rmx_ctx* ctx, uint64_t seed, int64_t row0, int32_t batch, int32_t n_fields,
                     int64_t num_rows, double exponent, int32_t* d_ids, void* stream);

/* Test hook: fill the LDS of every CU with a 32-bit pattern (e.g. 0x7FC00000, a NaN) on the stream, so a
 * kernel launched next that reads LDS it never wrote reads that pattern (tests/test_small_s3.py). */
int rmx_debug_fill_lds(rmx_ctx* ctx, uint32_t pattern, void* stream);

/* Test hook: fill the model's floating-point scratch buffers in HBM -- the inference workspace, the L-A
 * staging and the backward's state, each over its whole allocated capacity (the largest batch so far, not the
 * last one) -- with a 32-bit pattern on the stream (NULL: the context's stream), so a kernel of the next call
 * that reads a pad column or a row past its batch that the call did not write reads the pattern
 * (tests/test_workspace_leftovers.py).  Buffers of indices, offsets or pointers and state written once
 * (packed weights, biases, ...) are never touched: the hook cannot turn a leftover into a wild address.
 * *bytes_filled (nullable): how much was filled.  A model that has never run owns no scratch: RMX_OK, 0 bytes,
 * no device call.  NULL model: RMX_E_INVALID. */
int rmx_debug_poison_workspace(rmx_model* model, uint32_t pattern, void* stream, int64_t* bytes_filled);

/* Test hook (no device call): the device memory that the library's objects -- models, tables, optimisers,
 * shards, a running rmx_auc -- hold right now in this process: *bytes and *buffers (each nullable).  Memory
 * from rmx_malloc belongs to the caller and is not counted.  Both are back at their earlier reading once
 * everything created since has been destroyed (tests/test_device_memory.py). */
int rmx_debug_live_device_memory(int64_t* bytes, int64_t* buffers);

/* Test hook (host only, no GPU): the slice count S the training dW on the 208 x 208 tile uses for a
 * rows x N x K weight gradient on a device with ncu CUs.  S fixes the dW's fp32 summation order over the
 * slices, so gradients are bitwise reproducible across devices with the same CU count (every 256-CU
 * MI355X), not across CU counts.  Returns S (> 0) or RMX_E_INVALID. */
int rmx_debug_wgrad_slices(int64_t rows, int N, int K, int ncu);

/* Debug gather: d_w[n] = weights[ids[n]], d_emb[n*k+j] = emb[ids[n]][j] (makeWeights /
 * makeEmbeddings, ParRecModel.scala:279-306).  Bit-exact copies (as fp32 for a bf16 table). */
int rmx_gather(const rmx_table* t, int64_t n, const int32_t* d_ids, float* d_w, float* d_emb,
               void* stream);

/* L-B forward: d_ids[batch * nFields] (int32, device), d_out[batch] (device).
 * Requires rmx_model_set_mats / rmx_model_set_bias first.  Asynchronous on stream. */
int rmx_forward_ids(rmx_model* m, const rmx_table* t, int32_t batch, const int32_t* d_ids,
                    float* d_out, void* stream);

/* Per-stage timing of the last rmx_forward_ids calls made with timing enabled:
 * names/ms of up to cap stages (kernels) accumulated since enable. */
int rmx_model_set_timing(rmx_model* m, int enable);
int rmx_model_get_timing(rmx_model* m, char* names, int name_stride, float* ms, int cap, int* n,
                         int* calls);

/* Encoder-only launch (gather + first order + FM for DeepFM, first order otherwise):
 * d_y[batch] = y1 + y2 (DeepFM) / y1.  Used to measure the HBM-bound encoder alone. */
int rmx_encoder_ids(rmx_model* m, const rmx_table* t, int32_t batch, const int32_t* d_ids,
                    float* d_y, void* stream);

/* -------------------------------------------------------- sharded table ---- */
/* Hash-sharded table over nranks processes, one GPU each (BASELINE.json configs[3]): replaces
 * the column-range-partitioned Angel PS matrices and their sparse pulls (ParRecModel.scala:74-105,
 * :165-199).  owner(id) = p(id) mod nranks, local row = p(id) div nranks, p the keyed permutation of
 * rmx_shard_set_owner_hash (default key RMX_OWNER_HASH_DEFAULT).  One exchange per batch over
 * RCCL (grouped send/recv = all-to-all over xGMI): ids to owners, rows back.
 * At nranks > 1 the exchange has fixed-capacity buckets (~1.1 x ids / nranks per peer): every message
 * size is known on the host, so the exchange makes no host sync; ids past a bucket's capacity get their
 * rows in a second, counted round that every rank runs when any rank overflowed (each rank's header
 * carries its overflow flag).  The overflow check is made when the slot is consumed (or, for
 * rmx_forward_ids_sharded / rmx_shard_gather, after the forward / copy is queued, which then runs again).
 * An id outside [0, num_rows) reads a zero row on every path.
 * An exchange that fails on a rank at nranks > 1 (e.g. out of device memory while routing) leaves that
 * rank's collectives out of step with its peers': every later exchange on the shard returns RMX_E_COMM at
 * once.  Abort the shard on every rank (rmx_shard_abort, then rmx_shard_destroy) and create a new one;
 * peers already waiting in the failed exchange are released by their own abort (e.g. a watchdog).
 * The first exchange of a shard has no agreed bucket capacity yet, so all of its ids take the counted
 * overflow round (one extra round, once; timed under the "shard_exchange" stage) -- unless every rank
 * called rmx_shard_set_batch_hint with the same ids-per-batch figure first, which seeds that capacity.
 * CONTRACT CHANGE (round 3): the default owner function is the keyed permutation below, no longer
 * id mod nranks.  A caller that pre-partitions ids or rows must use rmx_owner_hash (or
 * rmx_shard_set_owner_hash(sh, 0) for id mod nranks). 
 * rmx_comm_unique_id: rank 0 creates the RCCL id (RMX_UNIQUE_ID_BYTES bytes) and the caller
 * broadcasts it (e.g. torch.distributed / MPI / Spark broadcast).  unique_id == NULL creates a
 * LOOPBACK shard: all nranks partitions live in this process on ctx's GPU and the exchange is
 * in-device (single-GPU testing of the routing at nranks > 1). */
#define RMX_UNIQUE_ID_BYTES 128
int rmx_comm_unique_id(void* out, size_t cap);
int rmx_shard_create(rmx_ctx* ctx, int64_t num_rows, int embedding_dim, int nranks, int rank,
                     const void* unique_id, rmx_shard** out);
int rmx_shard_destroy(rmx_shard* sh);
/* Abort the shard's RCCL communicator (ncclCommAbort) from any thread, e.g. a watchdog while an
 * exchange waits for a peer that never arrives: the pending exchange fails (or its kernels return)
 * and every later exchange returns RMX_E_COMM; only rmx_shard_destroy may follow.  Waits (at most 5 s)
 * for an exchange's host-side RCCL calls in flight on another thread to finish first, so no ncclSend /
 * ncclGroupEnd runs on the communicator while it is torn down.  A no-op returning RMX_OK for loopback and group shards. */
int rmx_shard_abort(rmx_shard* sh);
/* Owned rows from the same generator as rmx_table_fill_synthetic (bit-identical rows). */
int rmx_shard_fill_synthetic(rmx_shard* sh, uint64_t seed);
int64_t rmx_shard_local_rows(const rmx_shard* sh);
/* Owner function (before rmx_shard_fill_synthetic; every rank the same key): owner = p(id) mod
 * nranks, local row = p(id) div nranks with p a keyed pseudo-random permutation of [0, num_rows)
 * (4-round Feistel, cycle-walked), so strided or clustered id spaces spread evenly (the table is
 * HASH-sharded by default: key RMX_OWNER_HASH_DEFAULT); key 0 = the identity, owner = id mod nranks.
 * rmx_shard_owner_of: the rank owning id (-1 if out of range).  rmx_owner_hash: the same function
 * without a shard (host only): the owner of id, *local_row (nullable) its row there; -1 if id is
 * outside [0, num_rows) or the arguments are bad. */
#define RMX_OWNER_HASH_DEFAULT 0x5EED5A4D0C7A11EDULL
int rmx_shard_set_owner_hash(rmx_shard* sh, uint64_t key);
int64_t rmx_shard_owner_of(const rmx_shard* sh, int64_t id);
int64_t rmx_owner_hash(uint64_t key, int64_t num_rows, int nranks, int64_t id, int64_t* local_row);
/* Step 0 of the exchange: send each DISTINCT id of the batch once, as
 * ParRecModel.distinctIntIndices (ParRecModel.scala:337-345) before the pull; results are identical.
 * on: 0 off, 1 on, 2 auto (default: off at one rank; else on for a batch, then off for the next 63
 * batches when it removed fewer than 10 % of the ids, re-probed after them). */
int rmx_shard_set_dedupe(rmx_shard* sh, int on);
/* Seeds the first fixed-capacity exchange's bucket capacity from nnz, the ids one rank sends per batch
 * (B * nFields; the reference's batchSize * fields, ParRecModel.scala:165-199): ~1.1 nnz / nranks per
 * peer.  Collective by value: every rank must pass the same nnz before its first exchange.  Later
 * exchanges size their buckets from the previous one as before.  Without it the first exchange runs its
 * ids through the counted overflow round. */
int rmx_shard_set_batch_hint(rmx_shard* sh, int64_t nnz);
/* Ids this rank sent to owners in its last exchange (the distinct ids when deduplicating). */
int64_t rmx_shard_last_sent(const rmx_shard* sh);
/* Overflow rounds this shard has run (fixed-capacity exchange at nranks > 1: an id past its bucket's
 * capacity on any rank); -1 for a NULL shard. */
int64_t rmx_shard_overflow_rounds(const rmx_shard* sh);
/* Collective (every rank calls it): d_w[i] = w[ids[i]], d_emb[i*k+j] = emb[ids[i]][j] gathered
 * from the owners (makeWeights / makeEmbeddings through the exchange).  Bit-exact copies. */
int rmx_shard_gather(rmx_shard* sh, int64_t n, const int32_t* d_ids, float* d_w, float* d_emb,
                     void* stream);
/* In-process exchange group: nranks VIRTUAL ranks in one process (one host thread, context and
 * stream each, all on one GPU or several).  A shard created on a group runs the same exchange
 * schedule as the RCCL one (counts, ids to owners, owner gather, rows back, own bucket local), with
 * every grouped send/recv replaced by a device copy from the peer's posted buffer; the ranks
 * rendezvous inside each grouped step, so every rank must make the same collective calls, each from
 * its own thread (a rank missing for 120 s fails the step with RMX_E_COMM).  Used to run the
 * N > 1 exchange on a single GPU.  The group lives until it and all its shards are destroyed. */
int rmx_group_create(int nranks, rmx_group** out);
int rmx_group_destroy(rmx_group* g);
int rmx_shard_create_group(rmx_ctx* ctx, int64_t num_rows, int embedding_dim, rmx_group* group, int rank,
                           rmx_shard** out);
/* Collective: L-B forward of this rank's batch (d_ids [batch * nFields]) over the sharded table
 * (exchange + forward on one stream, through pull slot 0). */
int rmx_forward_ids_sharded(rmx_model* m, rmx_shard* sh, int32_t batch, const int32_t* d_ids,
                            float* d_out, void* stream);
/* The same split in two, so batch i + 1's exchange overlaps batch i's forward (the reference's pull*
 * then forward, ParRecModel.scala:165-199 / :279-306):
 *   rmx_shard_pull     (collective) exchange n ids into pull slot 0 or 1 on `stream`;
 *   rmx_forward_pulled forward of the batch in that slot on `stream` (typically another stream: it
 *                      waits for the pull on the device, and the slot's next pull waits for it).
 * A slot holds one pull until its forward consumes it (a second pull into it fails RMX_E_INVALID). */
int rmx_shard_pull(rmx_shard* sh, int64_t n, const int32_t* d_ids, int slot, void* stream);
int rmx_forward_pulled(rmx_model* m, rmx_shard* sh, int32_t batch, int slot, float* d_out, void* stream);
/* Training on the sharded table: the reference's optimize* (ParRecModel.scala:348-517) is pull, forward and
 * backward, then push to the partitioned PS matrices (pushWeightBiasEmbeddingMats, :225-253).
 * rmx_backward_pulled: the counterpart of rmx_forward_pulled -- one training pass (rmx_backward_ids' outputs and
 * layout: per nonzero of this rank's batch, the loss the mean BCE over its `batch` rows) over the rows in the pull
 * slot, which it consumes.  Same checks as rmx_forward_pulled (empty slot RMX_E_INVALID, another id count
 * RMX_E_SHAPE, model not fp32 RMX_E_INVALID, k mismatch RMX_E_SHAPE).  Every output equals rmx_backward_ids on a
 * replicated table holding the same rows, bit for bit, with the pull's dedupe on or off. */
int rmx_backward_pulled(rmx_model* m, rmx_shard* sh, int32_t batch, int slot, const float* d_targets,
                        float* d_g_bias, float* d_g_weights, float* d_g_embedding, float* d_g_mats,
                        float* d_loss, void* stream);
/* The push: an optimiser on a shard (the same rmx_optim type; rmx_optim_destroy before its model and shard,
 * rmx_optim_steps, and the mats / bias outputs of rmx_optim_state_ptrs work as for a table; its d_weights /
 * d_embedding outputs are NULL).  Argument checks as rmx_optim_create with the shard in the table's place, all
 * before any device or collective call.  State: zero-initialised [local rows][k] and [local rows] per partition
 * held here (a loopback shard holds nranks), mats_len and 1 as for a table; rmx_optim_shard_state_ptrs returns
 * partition `part`'s (0, except on a loopback shard), indexed by the local row of rmx_owner_hash.
 * rmx_optim_apply on such an optimiser is COLLECTIVE: every rank calls it for the same step with its own batch's
 * ids and per-nonzero gradients, the same groups NULL or non-NULL on every rank.  The result is fixed by the
 * sharded summation order above.  Protocol (csrc/shard.hip): the nonzeros bucketed by owner in
 * nonzero order, bucket sizes to the peers and ONE host sync on them (as the counted pull), the rows to their
 * owners, the replicated table's ordered sum and update there; g_mats / g_bias to every peer, added in rank order.
 * A failed collective leaves the shard failed as a failed pull does (rmx_shard_abort, then a new shard).  One rank:
 * no exchange and no host sync beyond rmx_optim_apply's own.
 * rmx_train_step_sharded (collective): pull into slot 0 (which must be free), rmx_backward_pulled into
 * optimiser-owned buffers, apply; synchronous on return; *loss (host, nullable) = this rank's own mean BCE.
 * rmx_train_step_ids with a sharded optimiser, and rmx_train_step_sharded with a table's optimiser or another
 * shard's, fail with RMX_E_INVALID before any device call.
 * Out of scope: bf16, pre-aggregating per distinct id before the send (another summation order), a
 * fixed-capacity sync-free push.  The RCCL transport at nranks > 1 has not been
 * executed for the push either (it uses the pull's grouped send / recv only). */
int rmx_optim_create_sharded(rmx_model* m, rmx_shard* sh, int kind, const double* hyper, int n_hyper,
                             rmx_optim** out);
int rmx_optim_shard_state_ptrs(const rmx_optim* o, int part, int slot, void** d_weights, void** d_embedding);
int rmx_train_step_sharded(rmx_model* m, rmx_shard* sh, rmx_optim* o, int32_t batch, const int32_t* d_ids,
                           const float* d_targets, float* loss, void* stream);

/* ------------------------------------------- loading and saving parameters ---- */
/* Host ranges of rows into and out of a table, a shard and an optimiser's state: what a checkpoint, a warm start
 * or a real model's load needs (csrc/param_io.hip).
 * Host range convention (every call below): the host pointers address the first element of the id range
 * [id0, id0 + n).  RMX_LAYOUT_ROW_MAJOR: embedding[i*k + j], ld ignored.  RMX_LAYOUT_K_MAJOR: embedding[j*ld + i]
 * with ld >= n (ld = V and id0 = 0: the Angel PS matrix).  weights[i] is the first-order weight of row id0 + i.
 * weights and embedding may each be NULL: that part is left as it is.  n = 0 returns RMX_OK without a device call.
 * Every call first waits for earlier device work (a device synchronise: these are not per-batch calls) and is
 * synchronous on return.  A range streams in chunks of "io_chunk_rows" rows (rmx_set_tuning; default 262,144)
 * through two pinned host buffers and two device chunk buffers owned by the table or shard -- allocated at the
 * first call, sized by the knob and k only (never by V), counted by rmx_debug_live_device_memory, reused by later
 * calls and freed with the object; chunk c + 1's host copy and transfer are ordered so that they can run under chunk c's kernel.  Knob "io_nt" 1:
 * non-temporal stores in the scatter (default 0).  Both defaults from the A/Bs of DESIGN.md §13: the calls reach
 * 0.4-0.55 of a plain copy of the same bytes, bounded by the host copy into the pinned chunk.
 * Errors: NULL handle, n < 0, an unknown layout, K_MAJOR with ld < n: RMX_E_INVALID; id0 < 0 or id0 + n > V:
 * RMX_E_INDEX; every check runs before any device call and rmx_last_error names the argument.
 *
 * Replicated table (fp32 or bf16: an upload rounds to nearest even exactly as rmx_table_upload does, a download
 * widens exactly).  An upload also writes the touched rows of the line copy (knob "table_lines"). */
int rmx_table_upload_rows(rmx_table* t, int64_t id0, int64_t n, const float* weights, const float* embedding,
                          int layout, int64_t ld);
int rmx_table_download_rows(const rmx_table* t, int64_t id0, int64_t n, float* weights, float* embedding,
                            int layout, int64_t ld);
/* Sharded table.  LOCAL calls, not collective: a row is kept (upload) or returned (download) only when its owner
 * partition lives in this shard object -- every partition of a loopback shard, else `rank`'s; owner = p(id) mod
 * nranks, local row = p(id) div nranks under the shard's owner function.  Other rows are skipped on upload
 * (*stored, nullable: the rows kept); on download their host elements are NOT written, owned[i] (nullable) says
 * which rows were and *found (nullable) counts them.  So every rank may be handed the whole table and keeps its
 * share (a loader that pre-partitions with rmx_owner_hash hands each rank less), at any nranks, without RCCL.
 * An upload fixes the owner function as a fill does (rmx_shard_set_owner_hash is refused afterwards).  A row
 * never uploaded reads as zeros; a line's pad floats and the partition's extra zero row stay zero.  Both calls
 * return RMX_E_INVALID while a pull slot holds an unconsumed pull (a direct slot reads the partition in place). */
int rmx_shard_upload_rows(rmx_shard* sh, int64_t id0, int64_t n, const float* weights, const float* embedding,
                          int layout, int64_t ld, int64_t* stored);
int rmx_shard_download_rows(rmx_shard* sh, int64_t id0, int64_t n, float* weights, float* embedding,
                            int layout, int64_t ld, uint8_t* owned /* [n], nullable */, int64_t* found);
/* Optimiser state, of a table's optimiser or a shard's (ownership as above; for a table every row is owned).
 * slot 0: v / s / m, slot 1: Adam's v.  A slot the kind does not have (slot 1 of Momentum, any slot of SGD), the
 * embedding state of LR and the first-order state of DNN: RMX_E_INVALID.  _dense: the [mats_len] and [1] state of
 * mats and the bias (each nullable).  rmx_optim_set_steps: the step count t >= 0 (the next apply uses t + 1).
 * With the rows, mats and bias restored too, a resumed run repeats the uninterrupted one bit for bit. */
int rmx_optim_state_upload_rows(rmx_optim* o, int slot, int64_t id0, int64_t n, const float* weights,
                                const float* embedding, int layout, int64_t ld, int64_t* stored);
int rmx_optim_state_download_rows(rmx_optim* o, int slot, int64_t id0, int64_t n, float* weights, float* embedding,
                                  int layout, int64_t ld, uint8_t* owned, int64_t* found);
int rmx_optim_state_upload_dense(rmx_optim* o, int slot, const float* mats /* [mats_len] */, const float* bias);
int rmx_optim_state_download_dense(rmx_optim* o, int slot, float* mats, float* bias);
int rmx_optim_set_steps(rmx_optim* o, int64_t t);
/* Test / bench hooks: the gather and the scatter kernel alone.  Rows [id0, id0 + n) (n > 0, at most one chunk of
 * "io_chunk_rows") are gathered into a device chunk, then `iters` gathers and `iters` scatters of that chunk are
 * timed by events: *get_ms / *put_ms (each nullable) = ms per launch.  The scatters store what the rows already
 * hold, so the table or shard is unchanged.  layout: the chunk's form on the device (K_MAJOR: transposed through
 * LDS).  Checks as the row calls. */
int rmx_debug_table_row_kernels(rmx_table* t, int64_t id0, int64_t n, int iters, int layout, float* get_ms,
                                float* put_ms);
int rmx_debug_shard_row_kernels(rmx_shard* sh, int64_t id0, int64_t n, int iters, int layout, float* get_ms,
                                float* put_ms);

/* ---- samples: native LIBSVM / LIBFFM parser (host, multi-threaded) ----
 * Replaces SampleParser.parse (yr/data/SampleParser.scala:14-85) for text in memory (one sample per
 * '\n'-terminated line): rows[nnz] = line index, cols[nnz] = id - 1, values[nnz], targets[lines] =
 * labels, fields[nnz] (LIBFFM only).  Malformed lines fail with RMX_E_INVALID naming the line, where
 * the reference throws NumberFormatException / ArrayIndexOutOfBoundsException.  nthreads <= 0:
 * all hardware threads.  The arrays stay valid until rmx_samples_free. */
int rmx_samples_parse(const char* text, size_t len, int format, int nthreads, rmx_samples** out);
int rmx_samples_free(rmx_samples* s);
int64_t rmx_samples_lines(const rmx_samples* s);
int64_t rmx_samples_nnz(const rmx_samples* s);
const int64_t* rmx_samples_rows(const rmx_samples* s);
const int64_t* rmx_samples_cols(const rmx_samples* s);
const float* rmx_samples_values(const rmx_samples* s);
const float* rmx_samples_targets(const rmx_samples* s);
const int64_t* rmx_samples_fields(const rmx_samples* s);  /* NULL for LIBSVM */
/* ids [lines][n_fields] (int32, ParRecModel.scala:342 .toInt) of a regular batch (every line has
 * exactly n_fields pairs: the models' Reshape(B, F, k)); RMX_E_SHAPE otherwise. */
int rmx_samples_ids(const rmx_samples* s, int32_t n_fields, int32_t* ids, int64_t cap);

#ifdef __cplusplus
}
#endif
#endif
