// k_fused_s3.hip -- DeepFM's whole fp32 tower in one persistent row-owner kernel on the split GEMM (gfx950),
// BASELINE.json configs[1].
//
// Layer 1 (gathered rows, first order and FM fused: k_head_s3.hip), layer 2 and layer 3 + the output dot and
// the head (k_tail_s3.hip) of DeepFM (model/encoder/HigherOrderEncoder.scala:34-59: three Linear(. -> 400) +
// ReLU over x = Reshape(B, F k) of the gathered embeddings, ParRecModel.scala:279-306; first order
// bnn/Scatter.scala:17-36; FM SecondOrderEncoder.scala:19-34; head DeepFM.scala:54-80: CAddTable + Sigmoid):
//   h1 = ReLU(x W1^T + b1), h2 = ReLU(h1 W2^T + b2)        both in the wave's registers, never in HBM
//   y  = sum_n ReLU(h2 W3^T + b3)[n] wo[n] + bo;  p = sigmoid((y1 + y2) + y + beta)
// Why: as head + tail, layer 1 wrote h1 (109 MB at B = 65,536) in one burst per round of
// blocks and the tail read it back through its own LDS-DMA ring, in a second launch.  With the operands
// swapped (D = W x^T, k_rowown.hpp), a lane holds outputs n = 16 t + 4 g .. + 3 of its sample -- exactly the
// K values lane group g feeds the next layer's split step (K = 32 c + 16 h + 4 g + q) -- so layer 1's
// accumulators ARE layer 2's B operand after bias + ReLU, as h2 already was for layer 3 in the tail.  The
// only HBM traffic left is the ids, the gathered rows + first-order weights, the L2-resident weight planes
// and p.
//
// Per row block (128 rows, a wave owns 16 of them and all 416 columns), one 3-slot weight ring, one barrier
// per unit (one K step x one column half), validated ONE UNIT AHEAD:
//   - a wave issues its five plane DMAs of unit U + 2 at tiles 0 .. 4 of unit U, into the slot of unit U - 1
//     (every wave read it before the barrier at the head of U); every other vector-memory instruction of the
//     unit comes after them (vmcnt retires in order);
//   - the wait at the head of unit U + 1 leaves in flight only those other instructions -- 4 after a layer-1
//     half-0 unit (1 id + 2 row + 1 weight DMA), 2 after layer 2's first unit (b2), otherwise 0 -- so the
//     wave's planes of U + 2 have landed, and the barrier proves U + 2 for every wave (U + 1 was proven one
//     barrier earlier; the prologue proves units 0 and 1);
//   - so the weight-fragment prefetch does not stop at a unit's end: at its last tiles a wave reads the first
//     fragments of the next unit (q_unit_ring, k_rowown.hpp), reaches the barrier with them in registers or
//     in flight, and issues tile 0's MFMAs without a refill.  Before, the barrier at the head of U was what
//     made U readable, and all eight waves left it with an empty fragment pipeline, 92 times per row block.
//   The fragment registers rotate (tile t in register set (phase + t) mod (PF + 1)), and the phase per unit is
//   a template argument: layers 2 and 3 are unrolled, so the ring is carried through layer 2's 26 units and
//   through each half of layer 3; layer 1's loop is rolled and its 25-tile K step shifts the phase by one, so
//   there the ring restarts at every half-0 unit (whose head forms the step's A operand after the barrier
//   anyway) and is carried into the half-1 unit.  Nothing is carried across a layer boundary or a row block:
//   23 restarts per row block at F = 39 instead of 92.
//   The price: the planes' lead over their wait falls from ~1.5 units to one unit less the five-tile spread
//   (they are L2 / Infinity-Cache resident).  Measured: DESIGN.md section 4, profiles/ring/.
//   layer 1: 2 KS units -- (c, half 0) then (c, half 1), the A operand (two fields' gathered rows) split once
//            per K step; ids three steps ahead and rows + first-order weights one step ahead (k_head_s3.hip),
//            running on across row blocks: the next block's first rows land during this block's last steps
//   layer 2: 26 units -- (c, half 0), (c, half 1) for c = 0 .. 12, the A operand h1 tiles 2c, 2c + 1 (from
//            registers; they die after step c, so h1 shrinks while acc2 fills: the peak is h1 + acc2 = 200
//            registers at c = 0)
//   layer 3: 26 units -- half 0's 13 steps, then half 1's, each half folding ReLU(. + b3) . wo into the
//            row's logit (k_tail_s3.hip q_layer3)
// Vector-memory instructions per unit: 9 in a layer-1 half-0 unit (1 id + 2 row + 1 weight DMA + 5 planes),
// 5 in every other unit -- every wait is a compile-time vmcnt.
//
// LDS: the ring (3 x 39,936) + per wave [2 A slots | 4 id slots | 2 weight slots] (8 x 4,864) + b3 | wo | b1
// (4,992) = 163,712 B.  b2 is DMA'd per row block into each wave's A slot that layer 1 no longer needs.
//
// Parity: each layer's products and K order are the head's / tail's, so h1, h2 and the logit's summands
// are the same fp32 values; the FM + first order are encoder_k16_kernel<1>'s arithmetic (bit-identical y1 +
// y2), and the head is the one function of every kernel (k_gemm.hpp out_head).  The predictions are therefore
// bitwise those of head + tail (tests/test_fused_s3.py), and held to 1e-5 against the fp64 oracle.
#include "k_rowown.hpp"

namespace rmx {
namespace {
using namespace rowown;

constexpr int kFKS2 = 13;                        // K steps of layers 2 and 3 (Kpad 416)
constexpr int kFPrm = 3 * kQN;                   // b3 | wo | b1 in LDS
constexpr size_t kFLds = (size_t)kQSlots * kQUnit + (size_t)kQW * kGWave + sizeof(float) * kFPrm;
static_assert(kFLds <= 160 * 1024, "LDS budget");
static_assert(sizeof(float) * kQN <= 2048, "b2 fits a wave's free A slot (f_b2_dma)");

// weight-fragment prefetch depth (column tiles) of the layer-2 units (2 measured the same, 0.3101-0.3102 vs
// 0.3093-0.3101 ms) and the layer-3 units (2 spilled 7 registers)
#ifndef RMX_FUSED_PF2
#define RMX_FUSED_PF2 1
#endif
#ifndef RMX_FUSED_PF3
#define RMX_FUSED_PF3 1
#endif

// Diagnostic builds only (tools/diag_fused.py; never set in librmx.so): bit 1 s_memtime stamps of block 0's
// waves at the layer boundaries of its first row blocks and at every layer-1 unit of row block 1, s_memrealtime
// at the kernel's start and end (the clock); timing probes with wrong results: bit 2 layer 1's row gathers
// from a fixed (cached) address, bit 4 no row / weight gathers in layer 1 at all
#ifndef RMX_FUSED_DIAG
#define RMX_FUSED_DIAG 0
#endif
#if RMX_FUSED_DIAG & 1
constexpr int kFDiagIt = 4, kFDiagPh = 6;
__device__ unsigned long long g_fused_t[kQW][kFDiagIt][kFDiagPh];  // [wave][row block][phase]
__device__ unsigned long long g_fused_clk[kQW][4];                   // memtime / memrealtime at start, end
__device__ unsigned long long g_fused_u[kQW][2 * kGMaxF];            // row block 1's layer-1 units, at entry
// one lane's vector store (the value and the address depend on the lane: never a scalar-cache store)
__device__ __forceinline__ void f_stamp(unsigned long long* dst, int lane, unsigned long long v) {
  int l = lane;
  asm volatile("" : "+v"(l), "+v"(v));
  if (l == 0) dst[l] = v;
}
#define F_USTAMP(it, u)                                                                                  \
  do {                                                                                                   \
    if (blockIdx.x == 0 && (it) == 1) f_stamp(&g_fused_u[w][u], lane, __builtin_amdgcn_s_memtime());     \
  } while (0)
#define F_STAMP(it, ph)                                                                                  \
  do {                                                                                                   \
    if (blockIdx.x == 0 && (it) < kFDiagIt) f_stamp(&g_fused_t[w][it][ph], lane, __builtin_amdgcn_s_memtime()); \
  } while (0)
// Inside one unit (row block 1 of block 0: layer 1's (kFProbeC1, half 0) and layer 2's (kFProbeC2, half 0)):
// 0 before q_enter, 1 after its barrier, 2 at the issue of the first MFMA (tile 0's fragments landed), 3 after
// the last MFMA.  Stores 0 .. 2 are older than the unit's plane DMAs, so the next q_enter's count still covers
// what it must; store 3 makes that one wait stricter by one DMA (the unit after the probed one).
constexpr int kFProbeC1 = 10, kFProbeC2 = 6;
__device__ unsigned long long g_fused_r[kQW][2][4];  // [wave][layer 1 / layer 2][point]
__device__ unsigned long long g_fused_rx[kQW];        // (the stamps of the units that are not probed)
struct FProbe {
  bool on;
  int w, lane, kind;
  template <int PEND>
  __device__ __forceinline__ void at(int i) const {
    // (no branch: a wave-uniform branch inside the unit made the compiler spill 88 VGPRs; every other unit of
    // this place in the code stamps into a dummy word)
    unsigned long long t;
    asm volatile("s_waitcnt lgkmcnt(%1)\n\ts_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) : "n"(PEND) : "memory");
    f_stamp(on ? &g_fused_r[w][kind][i] : &g_fused_rx[w], lane, t);
  }
};
template <class L>
struct FProbed {
  using probe_tag = void;
  const L& l;
  const FProbe& pr;
  __device__ __forceinline__ void operator()(int t) const { l(t); }
  template <int PEND>
  __device__ __forceinline__ void first() const {
    pr.template at<PEND>(2);
  }
  __device__ __forceinline__ void last() const { pr.template at<15>(3); }
};
#define F_PROBE_AT(pr, i) (pr).template at<15>(i)
#else
#define F_STAMP(it, ph) \
  do {                  \
  } while (0)
#define F_USTAMP(it, u) \
  do {                  \
  } while (0)
#define F_PROBE_AT(pr, i) \
  do {                    \
  } while (0)
#endif
// the extra functor of a probed unit: wrapped in diagnostic builds, itself otherwise
#if RMX_FUSED_DIAG & 1
#define F_PROBE_DECL(pr, cond, kind) const FProbe pr{(cond), w, lane, kind}
#define F_PROBED(x, pr) FProbed<decltype(x)>{x, pr}
#else
#define F_PROBE_DECL(pr, cond, kind) \
  do {                               \
  } while (0)
#define F_PROBED(x, pr) x
#endif

struct FusedS3Args {
  int M, F, KS, NU;       // KS = ceil(F / 2) layer-1 K steps; NU = 2 KS + 52 units per row block
  QRows rows;             // full / half row blocks (k_rowown.hpp)
  GatherArgs ga;          // ids [M][F], table, first-order weights (k_rowown.hpp)
  const bf16_t* W1;       // [KS][3][416][32] split planes (DenseLayer::W3)
  const float* b1;        // [416]
  const bf16_t* W2;       // [13][3][416][32]
  const float* b2;
  const bf16_t* W3;
  const float* b3;
  OutArgs oa;             // wo [416], bo, beta, out
  int prio;
};

// unit u of a row block -> its weight planes (wave-uniform)
__device__ __forceinline__ const bf16_t* f_unit_src(const FusedS3Args& p, int u) {
  const int l1 = 2 * p.KS;
  int c, half;
  const bf16_t* W;
  if (u < l1) {
    c = u >> 1;
    half = u & 1;
    W = p.W1;
  } else if (u < l1 + 2 * kFKS2) {
    const int v = u - l1;
    c = v >> 1;
    half = v & 1;
    W = p.W2;
  } else {
    const int v = u - l1 - 2 * kFKS2;
    half = v >= kFKS2 ? 1 : 0;
    c = v - half * kFKS2;
    W = p.W3;
  }
  return q_plane_src(W, c, half);
}

// the source of unit u + d (d <= 2), wrapping into the next row block's first units (the same weights)
__device__ __forceinline__ const bf16_t* f_ahead(const FusedS3Args& p, int u, int d) {
  const int v = u + d;
  return f_unit_src(p, v < p.NU ? v : v - p.NU);
}

// layer 1's unit (c, half) + 2 = (c + 1, half) of W1, or -- at the last K step -- layer 2's (0, half): W1 / W2
// are held in SGPRs across the loop and selected (f_ahead indexed the kernel arguments by a run-time unit, a
// scalar load whose lgkmcnt(0) wait also drained the unit's first LDS reads)
__device__ __forceinline__ const bf16_t* f_ahead1(const bf16_t* W1, const bf16_t* W2, int c, int KS, int half) {
  const bool l1 = c + 1 < KS;
  const bf16_t* W = l1 ? W1 : W2;
  const int cc = l1 ? c + 1 : 0;
  return q_plane_src(W, cc, half);
}

// unit V (a compile-time constant after unrolling) of layers 2 + 3 (V < 52), or V - 52 of the next row block's
// layer 1: a kernel-argument pointer made opaque at its use plus a constant offset -- formed from the
// runtime KS, or hoisted out of the row-block loop, the 52 unit sources spilled (SGPRs into VGPR lanes)
__device__ __forceinline__ const bf16_t* f_src23(const FusedS3Args& p, int V) {
  const bf16_t* W = V < 2 * kFKS2 ? p.W2 : (V < 4 * kFKS2 ? p.W3 : p.W1);
  asm volatile("" : "+s"(W));
  int c, half;
  if (V < 2 * kFKS2) {
    c = V >> 1;
    half = V & 1;
  } else if (V < 4 * kFKS2) {
    half = V - 2 * kFKS2 >= kFKS2 ? 1 : 0;
    c = V - 2 * kFKS2 - half * kFKS2;
  } else {
    c = (V - 4 * kFKS2) >> 1;
    half = (V - 4 * kFKS2) & 1;
  }
  return q_plane_src(W, c, half);
}

// Layer 1's row / weight DMAs from ids already in registers (k_rowown.hpp g_row_dma_ids), with the timing
// probes of diagnostic builds (results wrong)
__device__ __forceinline__ void f_row_dma_ids(const GatherArgs& ga, char* wl, int s, int lane, const GRowIds& q,
                                              int part) {
#if RMX_FUSED_DIAG & 4  // no row / weight gathers in layer 1
  return;
#elif RMX_FUSED_DIAG & 2  // every gather reads the lane's own row of the table's first 16 (cached)
  if (part < 2) {
    int g = swz_slot(lane >> 2, lane & 3);
    asm volatile("" : "+v"(g));
    lds_dma<16>(ga.table + ((int64_t)(lane >> 2) << ga.gsh) + 4 * g, wl + (s & 1) * 2048 + part * 1024);
    return;
  }
#endif
  g_row_dma_ids(ga, wl, s, lane, q, part);
}
// All three parts at once, each id read at its DMA (the prologue, the waves without rows).  This kernel's own
// copy, kept on purpose: k_rowown.hpp's g_row_dma forms every address before the first DMA, as k_head_s3.hip
// issues them, and built with that one this kernel spilled a second VGPR (scratch 8 -> 12 B per lane); built
// from g_row_ids + three g_row_dma_ids it kept its registers but not its code (the prologue and the loops of
// the waves without rows came out in another order).  With this copy the kernel is instruction for
// instruction what it was.
__device__ __forceinline__ void f_row_dma(const GatherArgs& ga, char* wl, int s, int lane) {
  const int* ids = reinterpret_cast<const int*>(wl + kGA + (s & 3) * 128);
  int r = lane >> 2, g = swz_slot(lane >> 2, lane & 3), lw = lane & 31;
  asm volatile("" : "+v"(r), "+v"(g), "+v"(lw));
  const float* zero16 = g_rmx_zero16;
  char* a = wl + (s & 1) * 2048;
  {
    const int id0 = ids[r];
    lds_dma<16>(id0 >= 0 ? ga.table + ((int64_t)id0 << ga.gsh) + 4 * g : zero16, a);
  }
  {
    const int id1 = ids[16 + r];
    lds_dma<16>(id1 >= 0 ? ga.table + ((int64_t)id1 << ga.gsh) + 4 * g : zero16, a + 1024);
  }
  {
    const int idw = ids[lw];
    if (lane < 32)
      lds_dma<4>(idw >= 0 ? ga.wtab + ((int64_t)idw << ga.wsh) : zero16, wl + kGA + kGId + (s & 1) * 128);
  }
}

// The biases of layers 1 and 2 come from LDS (round 6).  Read with scalar loads (round 5), the compiler
// reused one SGPR quad for all 25 tiles, so every s_load waited out its own round trip before the next:
// s_memtime stamps (tools/diag_fused.py) put the layer-1 epilogue at 8-14 k cycles per row block and the
// end of layer 2 likewise, ~6 % of the kernel.  b1 sits in the block's LDS beside b3 | wo (staged once per
// launch); b2 has no room there, so each wave DMAs it into its own A slot that layer 1's last step freed
// (slot (s - 1) & 1, untouched until the next row block's first rows land), during layer 2's first unit.
__device__ __forceinline__ void f_b2_dma(const FusedS3Args& p, char* wl, int s, int lane) {
  char* dst = wl + ((s - 1) & 1) * 2048;
  const float* zero16 = g_rmx_zero16;
  int l = lane;
  asm volatile("" : "+v"(l));
  lds_dma<16>(p.b2 + 4 * l, dst);                                  // bytes 0 .. 1023
  lds_dma<16>(l < kQN / 4 - 64 ? p.b2 + 256 + 4 * l : zero16, dst + 1024);  // 1024 .. 1663, then zeros
}

// f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>): a loop whose index is a constant expression
// (the fragment ring's phase per unit is a template argument of q_unit_ring)
template <class F, int... I>
__device__ __forceinline__ void f_static_for_seq(F&& f, std::integer_sequence<int, I...>) {
  (f(std::integral_constant<int, I>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void f_static_for(F&& f) {
  f_static_for_seq(f, std::make_integer_sequence<int, N>{});
}

// layer-3 half HF (column tiles 13 HF .. + 12; half 1 computes 12, tile 25 is padding): 13 units, one per
// K step, unrolled so that h2's tiles 2c, 2c + 1 are static registers (k_tail_s3.hip q_layer3)
template <int HF>
__device__ __forceinline__ void f_layer3(const FusedS3Args& p, char* lds, const float* prm, f32x4 (&h2)[kQNT],
                                         int& slot, int w, int lane, int lo, int fb, float& part) {
  f32x4 acc[kQUT];
#pragma unroll
  for (int t = 0; t < kQUT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  const f32x4 z = f32x4{0.f, 0.f, 0.f, 0.f};
  // the fragment ring is carried through the half's 13 units (each half starts its own: the output dot
  // stands between them)
  constexpr int NTU = HF == 0 ? kQUT : kQUT - 1;
  f32x4 bq[RMX_FUSED_PF3 + 1][3];
  f_static_for<kFKS2>([&](auto C) {
    constexpr int c = decltype(C)::value;
    q_enter<0>();
    bf16x8 ah, am, al;
    constexpr int c1 = 2 * c + 1 < kQNT ? 2 * c + 1 : 0;
    split3(h2[2 * c], 2 * c + 1 < kQNT ? h2[c1] : z, ah, am, al);
    const int dslot = q_dslot(slot);
    const char* ub = lds + slot * kQUnit;
    slot = q_next(slot);
    const bf16_t* src = f_src23(p, 2 * kFKS2 + HF * kFKS2 + c + 2);
    q_unit_ring<NTU, 0, kQUT, RMX_FUSED_PF3, (c * NTU) % (RMX_FUSED_PF3 + 1), c == 0, c + 1 < kFKS2>(
        ub, lds + slot * kQUnit, fb, ah, am, al, acc, bq, src, lds, dslot, w, lo);
  });
  q_dot_half<HF>(acc, prm, prm + kQN, lane >> 4, part);
}

__global__ __launch_bounds__(kQThreads, 1) void tower_fused_s3_kernel(FusedS3Args p) {
  extern __shared__ __attribute__((aligned(16))) char fsmem[];
  char* lds = fsmem;
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, r16 = lane & 15;
  char* wl = fsmem + kQSlots * kQUnit + w * kGWave;  // this wave's rows / ids / weights
  float* prm = reinterpret_cast<float*>(fsmem + kQSlots * kQUnit + kQW * kGWave);  // b3 | wo | b1
  const int nit = p.rows.nit(blockIdx.x);
  const int KS = p.KS;
  const OutArgs& oa = p.oa;
  // knob "fused_prio" (timing A/B): the second-dispatched half of the waves at priority 1 (MI355X_MICROARCH.md,
  // two waves per SIMD item 4)
  if (p.prio && w >= kQW / 2) __builtin_amdgcn_s_setprio(1);
#if RMX_FUSED_DIAG & 1
  if (blockIdx.x == 0) {
    f_stamp(&g_fused_clk[w][0], lane, __builtin_amdgcn_s_memtime());
    f_stamp(&g_fused_clk[w][1], lane, __builtin_amdgcn_s_memrealtime());
  }
#endif

  for (int i = tid; i < 2 * kQN; i += kQThreads) {
    const int a = i / kQN, n = i - a * kQN;
    const float* src = a == 0 ? p.b3 : oa.wo;
    prm[i] = src ? src[n] : 0.f;
  }
  // (a separate loop: a third source in the select above hit "illegal VGPR to SGPR copy" in the compiler)
  for (int i = tid; i < kQN; i += kQThreads) prm[2 * kQN + i] = p.b1[i];
  Q_LANE_LO(lo, lane);
  const int fb = q_fbase(lane);

  // the wave's layer-1 steps s = 0, 1, ... of the gathered-A stream run on over its row blocks (k_rowown.hpp)
  auto id_dma = [&](int s) { g_id_dma_step(p.ga.ids, p.M, p.F, p.rows, KS, wl, s, w, lane); };
  if (nit > 0) {
    for (int i = 0; i < 3; ++i) id_dma(i);
    q_drain();
    f_row_dma(p.ga, wl, 0, lane);
    Q_PROLOGUE(f_unit_src(p, 0), f_unit_src(p, 1), lds, w, lo);
  }
  q_meet();

  int slot = 0, s = 0;
  // Every wave runs one schedule: the unit's five plane DMAs at tiles 0 .. 4, layer 1's id / row / weight DMAs at
  // tiles 6, 8, 10, 11 of the half-0 unit, b2's at the last tile of layer 2's first unit -- the planes must be
  // the oldest of the unit's vector-memory instructions (header: the static waits).  The knob "fused_dma_split"
  // of rounds 5 / 6 (which wave half issued at which tiles) has no schedule of its own any more: 0, 1 and 2 are
  // accepted and run this one.
  for (int it = 0; it < nit; ++it) {
    int row0, nw;
    p.rows.desc(blockIdx.x, it, row0, nw);
    if (w >= nw) {
      // a half block's waves 4 .. 7: the same units, barriers and DMAs in the same order (ids of no rows), no
      // fragment reads, no MFMAs -- one branch per row block (per-unit branches spilled the accumulators).
      // (b2 is not DMA'd here, so the wait after layer 2's first unit is this wave's own count, 0)
#pragma unroll 1
      for (int c = 0; c < KS; ++c, ++s) {
        q_enter<0>();
        int dslot = q_dslot(slot);
        q_dma_only(f_ahead(p, 2 * c, 2), lds, dslot, w, lo);
        __builtin_amdgcn_sched_barrier(0);
        id_dma(s + 3);
        f_row_dma(p.ga, wl, s + 1, lane);
        __builtin_amdgcn_sched_barrier(0);
        slot = q_next(slot);
        q_enter<4>();  // 1 id + 2 row + 1 weight DMA, issued after the planes
        dslot = q_dslot(slot);
        q_dma_only(f_ahead(p, 2 * c + 1, 2), lds, dslot, w, lo);
        slot = q_next(slot);
      }
#pragma unroll 1
      for (int u = 2 * KS; u < p.NU; ++u) {
        q_enter<0>();
        const int dslot = q_dslot(slot);
        q_dma_only(f_ahead(p, u, 2), lds, dslot, w, lo);
        slot = q_next(slot);
      }
      continue;
    }
    // ---- layer 1 (+ first order + FM): units (c, half 0), (c, half 1) ----
    F_STAMP(it, 0);
    f32x4 h1[kQNT];
#pragma unroll
    for (int t = 0; t < kQNT; ++t) h1[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 fs = f32x4{0.f, 0.f, 0.f, 0.f}, fq = fs;
    float y1 = 0.f;
    bf16x8 ah, am, al;
    // step ss's A operand from its rows in A slot ss & 1: FM sums + first order (field order) and the split
    auto prep = [&](int ss) {
      int o = r16 * 64 + swz_slot(r16, g) * 16;
      asm volatile("" : "+v"(o));
      const char* a = wl + (ss & 1) * 2048;
      const f32x4 a0 = *reinterpret_cast<const f32x4*>(a + o);
      const f32x4 a1 = *reinterpret_cast<const f32x4*>(a + 1024 + o);
      const float* wr = reinterpret_cast<const float*>(wl + kGA + kGId + (ss & 1) * 128);
      {
#pragma clang fp contract(off)
        fm_accum(a0, a1, fs, fq);  // (SecondOrderEncoder sums, field order, k_gemm.hpp)
        y1 += wr[r16];             // first order in field order (encoder_k16_kernel<0>)
        y1 += wr[16 + r16];
      }
      split3(a0, a1, ah, am, al);
    };
    const bf16_t* W1 = p.W1;
    const bf16_t* W2 = p.W2;
    asm volatile("" : "+s"(W1), "+s"(W2));  // (loaded once per row block, selected per unit)
    // (forming step s + 1's A at the end of step s's half-1 unit, before the barrier, measured the same:
    // 0.3086-0.3097 vs 0.3094-0.3098 ms, profiles/r05/ab_fused.txt -- not kept)
    // The fragment ring restarts at every half-0 unit and is carried into the half-1 unit: a 13 + 12-tile K step
    // shifts the three-register rotation by one, and this loop is rolled (KS is a run-time value).  Unrolling it
    // by three with a remainder would carry the ring through the whole layer; not built -- the half-0 head
    // forms the step's A operand (rows, FM, split) after the barrier anyway.
    f32x4 bq1[3][3];
#pragma unroll 1
    for (int c = 0; c < KS; ++c, ++s) {
      F_PROBE_DECL(pr1, blockIdx.x == 0 && it == 1 && c == kFProbeC1, 0);
      F_PROBE_AT(pr1, 0);
      q_enter<0>();  // previous unit: (c - 1, half 1) or the previous row block's last layer-3 unit: planes only
      F_USTAMP(it, 2 * c);
      F_PROBE_AT(pr1, 1);  // (after the unit stamp's own store: the gap to the first MFMA is clean)
      // step s + 1's ids landed two steps ago (its id DMA rode step s - 2; every q_enter since waited for it)
      const GRowIds nid = g_row_ids(wl, s + 1, lane);
      prep(s);
      int dslot = q_dslot(slot);
      // the ids (3 steps ahead), rows and weights (1 step ahead) ride tiles 6, 8, 10, 11 of the unit's MFMA
      // stream, after its 5 plane DMAs: an LDS-DMA issue can hold its wave ~100-200 cycles, and four of them
      // ahead of the unit's first MFMA (k_head_s3.hip's order) cost 2 % (0.3142-0.3162 vs 0.3088-0.3111 ms)
      const int sn = s;
      auto extra = [&](int t) {
        if (t == 6) id_dma(sn + 3);
        if (t == 8) f_row_dma_ids(p.ga, wl, sn + 1, lane, nid, 0);
        if (t == 10) f_row_dma_ids(p.ga, wl, sn + 1, lane, nid, 1);
        if (t == 11) f_row_dma_ids(p.ga, wl, sn + 1, lane, nid, 2);
      };
      const char* ub0 = lds + slot * kQUnit;
      slot = q_next(slot);
      const char* ub1 = lds + slot * kQUnit;
      q_unit_ring<kQUT, 0, kQNT, 2, 0, true, true>(ub0, ub1, fb, ah, am, al, h1, bq1, f_ahead1(W1, W2, c, KS, 0), lds, dslot,
                                                   w, lo, F_PROBED(extra, pr1));
      q_enter<4>();  // previous unit: 1 id + 2 row + 1 weight DMA after its planes
      F_USTAMP(it, 2 * c + 1);
      dslot = q_dslot(slot);
      q_unit_ring<kQNT - kQUT, kQUT, kQNT, 2, q_ring_phase<2>(0, kQUT), false, false>(
          ub1, ub1, fb, ah, am, al, h1, bq1, f_ahead1(W1, W2, c, KS, 1), lds, dslot, w, lo);
      slot = q_next(slot);
    }
    __builtin_amdgcn_sched_barrier(0);
    F_STAMP(it, 1);
    // first order + FM of the row (k_head_s3.hip's epilogue: encoder_k16_kernel<1>'s arithmetic)
    float pre;
    {
#pragma clang fp contract(off)
      float a = 0.f;
      float d[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) d[t] = fs[t] * fs[t] - fq[t];
#pragma unroll
      for (int gg = 0; gg < 4; ++gg)
#pragma unroll
        for (int t = 0; t < 4; ++t) a += __shfl(d[t], gg * 16 + r16);
      pre = y1 + 0.5f * (a / 16.0f);
    }
    asm volatile("" : "+v"(pre));  // (formed here: sunk to the head, its 16 shuffled terms were spilled)
    // h1 = ReLU(acc1 + b1), in place (b1 from LDS)
    {
      int o = 4 * g;
      asm volatile("" : "+v"(o));
#pragma unroll
      for (int t = 0; t < kQNT; ++t) h1[t] = relu4(h1[t] + *reinterpret_cast<const f32x4*>(prm + 2 * kQN + 16 * t + o));
    }
    // ---- layer 2: units (c, half 0), (c, half 1); h1 tiles 2c, 2c + 1 die after step c ----
    F_STAMP(it, 2);
    f32x4 h2[kQNT];
#pragma unroll
    for (int t = 0; t < kQNT; ++t) h2[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int sb2 = s;  // (b2 goes to A slot (sb2 - 1) & 1: f_b2_dma)
    // the fragment ring is carried through all 26 units (the phase of unit (c, half) is a constant)
    f32x4 bq2[RMX_FUSED_PF2 + 1][3];
    f_static_for<kFKS2>([&](auto C) {
      constexpr int c = decltype(C)::value;
      constexpr int kPh0 = (c * kQNT) % (RMX_FUSED_PF2 + 1), kPh1 = q_ring_phase<RMX_FUSED_PF2>(kPh0, kQUT);
      F_PROBE_DECL(pr2, blockIdx.x == 0 && it == 1 && c == kFProbeC2, 1);
      F_PROBE_AT(pr2, 0);
      q_enter<0>();
      F_PROBE_AT(pr2, 1);
      bf16x8 ah, am, al;
      const f32x4 z = f32x4{0.f, 0.f, 0.f, 0.f};
      constexpr int c1 = 2 * c + 1 < kQNT ? 2 * c + 1 : 0;
      split3(h1[2 * c], 2 * c + 1 < kQNT ? h1[c1] : z, ah, am, al);
      int dslot = q_dslot(slot);
      // unit (0, half 0) also DMAs b2 into this wave's free A slot, at its last tile (after the 5 plane DMAs)
      auto b2x = [&](int t) {
        if (c == 0 && t == kQUT - 1) f_b2_dma(p, wl, sb2, lane);
      };
      const char* ub0 = lds + slot * kQUnit;
      slot = q_next(slot);
      const char* ub1 = lds + slot * kQUnit;
      q_unit_ring<kQUT, 0, kQNT, RMX_FUSED_PF2, kPh0, c == 0, true>(ub0, ub1, fb, ah, am, al, h2, bq2, f_src23(p, 2 * c + 2),
                                                                    lds, dslot, w, lo, F_PROBED(b2x, pr2));
      q_enter<c == 0 ? 2 : 0>();  // (the 2 DMAs of b2 came after unit (0, half 0)'s planes)
      dslot = q_dslot(slot);
      slot = q_next(slot);
      q_unit_ring<kQNT - kQUT, kQUT, kQNT, RMX_FUSED_PF2, kPh1, false, c + 1 < kFKS2>(
          ub1, lds + slot * kQUnit, fb, ah, am, al, h2, bq2, f_src23(p, 2 * c + 3), lds, dslot, w, lo);
    });
    __builtin_amdgcn_sched_barrier(0);
    {
      // b2 from this wave's A slot (its DMA landed units ago: every later q_enter waited for it)
      // (the lane id made afresh by mbcnt: kept from the kernel's start, lane & 48 was spilled to scratch)
      const int ln = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
      int o = ((sb2 - 1) & 1) * 2048 + 16 * (ln >> 4);
      asm volatile("" : "+v"(o));
#pragma unroll
      for (int t = 0; t < kQNT; ++t) h2[t] = relu4(h2[t] + *reinterpret_cast<const f32x4*>(wl + o + 64 * t));
    }
    // ---- layer 3 + the output dot ----
    F_STAMP(it, 3);
    float part = 0.f;
    f_layer3<0>(p, lds, prm, h2, slot, w, lane, lo, fb, part);
    F_STAMP(it, 4);
    f_layer3<1>(p, lds, prm, h2, slot, w, lane, lo, fb, part);
    F_STAMP(it, 5);
    // ---- head: the four lane groups' columns, then bias, CAddTable, sigmoid (k_gemm.hpp out_head) ----
    part += __shfl_xor(part, 16);
    part += __shfl_xor(part, 32);
    // (lane made afresh, as for b2: the kernel-start r16 was spilled here, and its reload waited vmcnt(0) --
    // for every DMA in flight, the next row block's first units included)
    const int ln = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    const int m = row0 + w * 16 + (ln & 15);
    if (ln < 16 && m < p.M) {
      oa.out[m] = out_head(oa, part, false, 0.f, false, 0.f, true, pre);
    }
  }
  q_drain();  // (the next block's ids / rows, too)
#if RMX_FUSED_DIAG & 1
  if (blockIdx.x == 0) {
    f_stamp(&g_fused_clk[w][2], lane, __builtin_amdgcn_s_memtime());
    f_stamp(&g_fused_clk[w][3], lane, __builtin_amdgcn_s_memrealtime());
  }
#endif
}

}  // namespace

#if RMX_FUSED_DIAG & 1
// out: [8 waves][4 row blocks][6 stamps], [8 waves][4] (memtime, memrealtime at start and end), then
// [8 waves][80] row block 1's layer-1 unit entries, then [8 waves][2 units][4 points] inside two units
extern "C" int rmx_diag_fused(unsigned long long* out) {
  RMX_HIP(hipDeviceSynchronize());
  RMX_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_fused_t), sizeof(g_fused_t)));
  RMX_HIP(hipMemcpyFromSymbol(out + sizeof(g_fused_t) / 8, HIP_SYMBOL(g_fused_clk), sizeof(g_fused_clk)));
  RMX_HIP(hipMemcpyFromSymbol(out + (sizeof(g_fused_t) + sizeof(g_fused_clk)) / 8, HIP_SYMBOL(g_fused_u),
                              sizeof(g_fused_u)));
  RMX_HIP(hipMemcpyFromSymbol(out + (sizeof(g_fused_t) + sizeof(g_fused_clk) + sizeof(g_fused_u)) / 8,
                              HIP_SYMBOL(g_fused_r), sizeof(g_fused_r)));
  return RMX_OK;
}
#endif

// what the kernel itself relies on: F <= 40 fields of k = 16 into three 400-wide split-GEMM layers, b1 and b2
// present (they are read without a null check).  The launch checks this much; the path choice below asks for
// more -- a plain per-output bias, no bf16 planes, no extra columns -- as it always did.
static bool fused_s3_shape(const DenseLayer& L1, const DenseLayer& L2, const DenseLayer& L3, int F) {
  return F >= 1 && F <= kGMaxF && L1.W3 && L2.W3 && L3.W3 && L1.b && L2.b && L1.K == 16 * F && L1.Npad == kQN &&
         L2.Npad == kQN && L3.Npad == kQN && L2.K == 400 && L3.K == 400 && L1.N == 400 && L2.N == 400 && L3.N == 400;
}

bool tower_fused_s3_usable(const DenseLayer& L1, const DenseLayer& L2, const DenseLayer& L3, int M, int F, int k,
                           bool ids) {
  if (M <= 0 || !ids || k != 16 || !f32_split_enabled() || !fused_s3_shape(L1, L2, L3, F)) return false;
  if (L1.W16 || L2.W16 || L3.W16) return false;
  if (!(L1.N1 < 0 && L1.bias_mode == 1 && L1.K1 < 0)) return false;
  if (!((L2.Kpad + 31) / 32 == kFKS2 && (L3.Kpad + 31) / 32 == kFKS2 && L2.N1 < 0 && L3.N1 < 0 && L2.bias_mode == 1 &&
        L3.bias_mode == 1))
    return false;
  // knob "s3_fused": 0 off (head + tail), 1 (default) / 2 on.  Round 5 kept it to batches whose full 128-row
  // blocks fill every CU (B = 16,384: head + tail 154.4 M against the fused tower's 147.7 M then,
  // profiles/r05/ab_fused_batch.txt); after round 6's fused-tower work it wins at every batch the small-batch
  // kernels leave to it (they take B <= 8,192 first): B = 9,216 / 12,288 / 16,384 / 24,576 107 / 142 / 173 / 180 M
  // against head + tail's 90 / 119 / 152 / 157 M (profiles/r06/ab_fused_mid_batches.txt)
  return tuning_get("s3_fused", 1) != 0;
}

int launch_tower_fused_s3(hipStream_t s, const DenseLayer& L1, const DenseLayer& L2, const DenseLayer& L3, int M, int F,
                          const int32_t* ids, const float* table, int ld, const float* wtab, int wld,
                          const OutArgs& oa) {
  if (!ids || !oa.wo || !oa.out || !fused_s3_shape(L1, L2, L3, F)) {
    set_error("fp32 fused tower: needs a k = 16 gather (F <= 40, ids) into three 400-wide split-GEMM layers + head");
    return RMX_E_INVALID;
  }
  if (M <= 0) return RMX_OK;
  FusedS3Args p{};
  if (!gather_shifts(ld, wld, p.ga.gsh, p.ga.wsh)) {
    set_error("fp32 fused tower: table / weight strides must be powers of two");
    return RMX_E_INVALID;
  }
  int ncu = 0;
  RMX_HIP(cu_count(&ncu));
  RMX_HIP(hipFuncSetAttribute((const void*)tower_fused_s3_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)kFLds));
  p.M = M;
  int grid = 0;
  p.rows = q_rows(M, ncu, grid);
  p.F = F;
  p.KS = (F + 1) / 2;
  p.NU = 2 * p.KS + 4 * kFKS2;
  p.ga.ids = ids;
  p.ga.table = table;
  p.ga.wtab = wtab;
  p.W1 = L1.W3;
  p.b1 = L1.b;
  p.W2 = L2.W3;
  p.b2 = L2.b;
  p.W3 = L3.W3;
  p.b3 = L3.b;
  p.oa = oa;
  p.prio = tuning_get("fused_prio", 0);
  hipLaunchKernelGGL(tower_fused_s3_kernel, dim3(grid), dim3(kQThreads), kFLds, s, p);
  RMX_HIP(hipGetLastError());
  return RMX_OK;
}

}  // namespace rmx
