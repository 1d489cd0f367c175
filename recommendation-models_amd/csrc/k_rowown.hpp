// k_rowown.hpp -- the row-owner split-GEMM machinery of the fp32 tower kernels (gfx950).  Its users:
//   k_head_s3.hip   DeepFM layer 1 (gathered A):   the weight ring with q_unit, QRows, the gathered-A stream
//   k_tail_s3.hip   layers 2 + 3 + head:           the ring with q_unit, QRows, the stored-A stream, q_dot_half
//   k_layer_s3.hip  one 400 x 400 training layer:  the ring with q_unit, QRows, the stored-A stream, bits_set
//   k_fused_s3.hip  DeepFM's whole tower:          the ring with q_unit_ring (validated one unit ahead), QRows,
//                                                  the gathered-A stream, q_dot_half
// Each kernel keeps its own schedule: which unit of a row block reads which (W, K step, column half), and at
// which tiles its own vector-memory instructions ride; the pieces every schedule is made of live here, once.
// (k_small_s3.hip, the whole-tower kernel of small batches, is a different design and takes nothing from here.)
//
// A block of 8 waves (two per SIMD) owns 128 rows; a wave owns 16 rows and ALL 416 columns of a layer.
// The MFMA runs with the operands swapped (D = W x^T, v_mfma_f32_16x16x32_bf16 with the weight plane as
// A), so lane (r16, g) holds outputs n = 16 t + 4 g .. + 3 of its sample r16 -- the K values that lane
// group g feeds the next layer at the split engine's positions (k_gemm.hpp kPrecS3: step c, half h,
// K = 32 c + 16 h + 4 g + q).  The weights (fp32 pre-split into three bf16 planes, W3 [steps][3][416][32])
// stream through LDS in "units" of one K step x one column half (13 tiles x 3 planes x 1 KiB = 39 KiB), a
// 3-slot ring: unit U + 2's DMAs are issued during unit U, one per column tile, one barrier per unit.
#pragma once

#include "k_gemm.hpp"

namespace rmx {
namespace rowown {

constexpr int kQBM = 128;                    // rows per row block
constexpr int kQW = 8;                       // waves
constexpr int kQThreads = kQW * 64;
constexpr int kQNT = 25;                     // computed column tiles (N = 400)
constexpr int kQN = 416;                     // Npad: packed rows of W per plane and K step
constexpr int kQUT = 13;                     // column tiles per unit (one half of Npad)
constexpr int kQUnit = 3 * kQUT * 16 * 64;   // bytes per unit: 3 planes x 208 rows x 64 B = 39,936
constexpr int kQIns = kQUnit / 1024;         // 1-KiB DMA instructions per unit (39)
constexpr int kQQ = (kQIns + kQW - 1) / kQW; // per wave (5; wave 7's fifth repeats instruction 38)
constexpr int kQSlots = 3;
static_assert(kQQ == 5 && kQIns == 39, "the static vmcnt counts assume 5 weight DMAs per wave per unit");

// this wave's DMA q of a unit whose planes start at `src` into the slot at `dst` (LDS byte offset).
// Instruction ins = w + 8 q fills unit rows [16 ins, 16 ins + 16): plane ins / 13, tile ins % 13; lane L
// writes physical 16-B slot L & 3 of row L >> 2, so it loads logical slot swz_slot(row, L & 3) (the
// swizzle is an involution; the key of row 16 t + (L >> 2) depends on L only): lo = its element offset.
__device__ __forceinline__ void q_dma(const bf16_t* src, char* lds, int slot, int w, int q, int lo) {
  int ins = w + q * kQW;
  ins = ins < kQIns ? ins : kQIns - 1;
  const int pl = ins / kQUT, t = ins - pl * kQUT;
  int l = lo;
  asm volatile("" : "+v"(l));  // formed here: hoisted, the 130 per-unit sources of layer 3 spilled
  const bf16_t* s = src + (pl * kQN + t * 16) * 32 + l;
  lds_dma<16>(s, lds + slot * kQUnit + ins * 1024);
}

__device__ __forceinline__ int q_next(int s) { return s == kQSlots - 1 ? 0 : s + 1; }

// the ring's write slot during the unit in `slot`: unit U + 2's, (slot + 2) mod 3 -- the slot of unit U - 1,
// which every wave read before the barrier at the head of U
__device__ __forceinline__ int q_dslot(int slot) { return slot == 0 ? 2 : slot - 1; }

// `int lo` = the lane offset (bf16 elements) of the plane DMAs' sources: row L >> 2 of a tile, logical slot
// swz_slot(row, L & 3), 8 bf16 each (q_dma's lo).
// This and Q_PROLOGUE are macros, not functions, so that each kernel compiles to the code it had when it wrote
// them out: formed by an inlined function, the same values left three of the four kernels allocated
// differently from end to end (k_tail_s3.hip: 253 VGPRs for 254 on top of 258 spilled SGPRs; k_fused_s3.hip
// and k_layer_s3.hip: other registers throughout).
#define Q_LANE_LO(lo, lane)                                                  \
  int lo = ((lane) >> 2) * 32 + swz_slot((lane) >> 2, (lane) & 3) * 8; \
  asm volatile("" : "+v"(lo))

// the planes of K step c, column half `half` of a layer's split weights W [steps][3][416][32].  Which unit of
// a row block is which (W, c, half) is each kernel's schedule (its *_unit_src)
__device__ __forceinline__ const bf16_t* q_plane_src(const bf16_t* W, int c, int half) {
  return W + (int64_t)(c * 3 * kQN + half * kQUT * 16) * 32;
}

// everything this wave has issued has landed: before the block's first barrier, and at the kernel's end (the
// ring's trailing DMAs -- units 0 / 1 of a row block that does not exist -- land before the LDS is released)
__device__ __forceinline__ void q_drain() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// the two-unit fill of the ring (a block with row blocks): this wave's DMAs of units 0 and 1 (planes at src0 /
// src1) into slots 0 and 1
#define Q_PROLOGUE(src0, src1, lds, w, lo)                                                   \
  do {                                                                                       \
    _Pragma("unroll") for (int q_ = 0; q_ < kQQ; ++q_) q_dma(src0, lds, 0, w, q_, lo);       \
    _Pragma("unroll") for (int q_ = 0; q_ < kQQ; ++q_) q_dma(src1, lds, 1, w, q_, lo);       \
  } while (0)
// ... then they -- and whatever else the wave issued before (its first A rows / ids) -- land, and the block
// meets (its staged parameters are written, too).  q_enter's barrier covers the other waves' DMAs from then on.
__device__ __forceinline__ void q_meet() {
  q_drain();
  __syncthreads();
}

// per-lane byte offset of the weight fragments (row r16 of a tile, logical slot g), opaque so the
// fragment addresses are formed per use
__device__ __forceinline__ int q_fbase(int lane) {
  int fb = (lane & 15) * 64 + swz_slot(lane & 15, lane >> 4) * 16;
  asm volatile("" : "+v"(fb));
  return fb;
}

// no extra vector-memory instructions in a unit (q_unit's default)
struct QNoExtra {
  __device__ __forceinline__ void operator()(int) const {}
};

// Diagnostic builds only: an extra functor that declares `probe_tag` is called at the issue of the unit's first
// MFMA (first<PEND>(): PEND fragment reads of later tiles may stay in flight) and after its last (last())
// (k_fused_s3.hip's stamps); no functor of librmx.so has one.
template <class X, class = void>
struct q_has_probe : std::false_type {};
template <class X>
struct q_has_probe<X, std::void_t<typename X::probe_tag>> : std::true_type {};

// One unit: NT column tiles (local tiles 0 .. NT - 1 of the unit's half) of one K step.  acc[T0 + t] +=
// W_t h^T on the split planes (ah, am, al) of this wave's 16 rows; dma(q) issues the wave's q-th DMA of
// unit U + 2, one per tile.  The fragments of tile t + 2 are read while tile t's MFMAs run.  extra(t) may
// issue more vector-memory instructions at tile t (after that tile's plane DMA): a caller's own DMAs spread
// over the MFMA stream instead of issued ahead of it.
// The wave's five plane DMAs ride tiles 0 .. 4.
template <int NT, int T0, int NA, int PF = 2, class X = QNoExtra>
__device__ __forceinline__ void q_unit(const char* ub, int fb, const bf16x8& ah, const bf16x8& am, const bf16x8& al,
                                       f32x4 (&acc)[NA], const bf16_t* dsrc, char* lds, int dslot, int w, int lo,
                                       const X& extra = X()) {
  f32x4 bq[PF + 1][3];
  int fbu = fb;
  asm volatile("" : "+v"(fbu));
  auto ldb = [&](int t, f32x4* b) {
#pragma unroll
    for (int pl = 0; pl < 3; ++pl) b[pl] = *reinterpret_cast<const f32x4*>(ub + fbu + pl * (kQUT * 1024) + t * 1024);
  };
#pragma unroll
  for (int t = 0; t < PF; ++t) ldb(t, bq[t]);
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    if (t + PF < NT) ldb(t + PF, bq[(t + PF) % (PF + 1)]);
    static_assert(kQQ - 1 < kQUT - 1, "every unit (12 or 13 tiles) carries all its DMAs");
    if (t < kQQ) q_dma(dsrc, lds, dslot, w, t, lo);
    extra(t);
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (q_has_probe<X>::value) {
      if (t == 0) extra.template first<3 * PF>();
    }
    const f32x4* b = bq[t % (PF + 1)];
    const bf16x8 bh = __builtin_bit_cast(bf16x8, b[0]);
    const bf16x8 bm = __builtin_bit_cast(bf16x8, b[1]);
    const bf16x8 bl = __builtin_bit_cast(bf16x8, b[2]);
    f32x4 d = acc[T0 + t];
    // the engine's product order (k_gemm.hpp compute_step_s3), operands swapped: smallest terms first
    d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bm, am, d, 0, 0, 0);
    d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bh, al, d, 0, 0, 0);
    d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bl, ah, d, 0, 0, 0);
    d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bh, am, d, 0, 0, 0);
    d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bm, ah, d, 0, 0, 0);
    acc[T0 + t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bh, ah, d, 0, 0, 0);
    if constexpr (q_has_probe<X>::value) {
      if (t == NT - 1) extra.last();
    }
  }
}

// q_unit for a ring that is validated one unit ahead (k_fused_s3.hip): the barrier at the head of a unit has
// proven the NEXT unit too, so the fragment prefetch does not stop at the unit's last tiles -- it runs on
// into tiles 0 .. PF - 1 of the next unit (at `ubn`), and the wave reaches the next barrier with its first
// fragments in registers or in flight.  bq is the caller's fragment ring, carried from unit to unit: tile t's
// fragments sit in bq[(PH + t) % (PF + 1)], so the next unit's phase is q_ring_phase (every index stays a
// compile-time constant).  HEAD: the chain starts here (nothing was prefetched: read tiles 0 .. PF - 1 first,
// as q_unit does); CARRY: prefetch into the next unit (false in the chain's last unit).  The wave's five plane
// DMAs ride tiles 0 .. 4, ahead of everything extra(t) issues (callers use tiles >= 5): the wait at the next
// unit's head counts only those extras.  MFMA order per accumulator as in q_unit.
template <int PF>
constexpr int q_ring_phase(int ph, int nt) {
  return (ph + nt) % (PF + 1);
}
template <int NT, int T0, int NA, int PF, int PH, bool HEAD, bool CARRY, class X = QNoExtra>
__device__ __forceinline__ void q_unit_ring(const char* ub, const char* ubn, int fb, const bf16x8& ah, const bf16x8& am,
                                            const bf16x8& al, f32x4 (&acc)[NA], f32x4 (&bq)[PF + 1][3],
                                            const bf16_t* dsrc, char* lds, int dslot, int w, int lo,
                                            const X& extra = X()) {
  static_assert(PF >= 1 && PF < NT && PH >= 0 && PH <= PF, "fragment ring");
  int fbu = fb;
  asm volatile("" : "+v"(fbu));
  auto ldb = [&](const char* u, int t, f32x4* b) {
#pragma unroll
    for (int pl = 0; pl < 3; ++pl) b[pl] = *reinterpret_cast<const f32x4*>(u + fbu + pl * (kQUT * 1024) + t * 1024);
  };
  if constexpr (HEAD) {
#pragma unroll
    for (int t = 0; t < PF; ++t) ldb(ub, t, bq[(PH + t) % (PF + 1)]);
  }
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    if (t + PF < NT)
      ldb(ub, t + PF, bq[(PH + t + PF) % (PF + 1)]);
    else if constexpr (CARRY)
      ldb(ubn, t + PF - NT, bq[(PH + t + PF) % (PF + 1)]);
    if (t < kQQ) q_dma(dsrc, lds, dslot, w, t, lo);
    extra(t);
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (q_has_probe<X>::value) {
      if (t == 0) extra.template first<3 * PF>();
    }
    const f32x4* b = bq[(PH + t) % (PF + 1)];
    const bf16x8 bh = __builtin_bit_cast(bf16x8, b[0]);
    const bf16x8 bm = __builtin_bit_cast(bf16x8, b[1]);
    const bf16x8 bl = __builtin_bit_cast(bf16x8, b[2]);
    f32x4 d = acc[T0 + t];
    d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bm, am, d, 0, 0, 0);
    d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bh, al, d, 0, 0, 0);
    d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bl, ah, d, 0, 0, 0);
    d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bh, am, d, 0, 0, 0);
    d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bm, ah, d, 0, 0, 0);
    acc[T0 + t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bh, ah, d, 0, 0, 0);
    if constexpr (q_has_probe<X>::value) {
      if (t == NT - 1) extra.last();
    }
  }
}

// the DMAs of q_unit without its MFMAs: a wave that owns no rows this row block (a half block's waves
// 4 .. 7) keeps the ring and the static vmcnt counts
__device__ __forceinline__ void q_dma_only(const bf16_t* dsrc, char* lds, int dslot, int w, int lo) {
#pragma unroll
  for (int q = 0; q < kQQ; ++q) q_dma(dsrc, lds, dslot, w, q, lo);
}

// Row blocks of a persistent row-owner launch (grid G): full 128-row blocks, round-robin.  When the last
// round would leave at least half the CUs idle, its rows go out as 64-row half blocks instead: waves 0 .. 3
// own the rows, waves 4 .. 7 keep the weight ring and the barriers but run no MFMAs, so the round costs
// about half a round (B = 49,152 on 256 CUs: 1.5 rounds instead of 2; B = 16,384: half a round, not one).
struct QRows {
  int M, G, nfull, nhalf;  // nfull full blocks, then nhalf half blocks from row nfull * 128
  __device__ __forceinline__ int nf(int b) const { return b < nfull ? (nfull - 1 - b) / G + 1 : 0; }
  __device__ __forceinline__ int nit(int b) const { return nf(b) + (b < nhalf ? 1 : 0); }
  // iteration it of block b: first row and the number of waves that own rows (0: none -- past the end)
  __device__ __forceinline__ void desc(int b, int it, int& row0, int& nw) const {
    const int n = nf(b);
    if (it < n) {
      row0 = (b + it * G) * kQBM;
      nw = kQW;
    } else if (it == n && b < nhalf) {
      row0 = nfull * kQBM + b * (kQBM / 2);
      nw = kQW / 2;
    } else {
      row0 = M;
      nw = 0;
    }
  }
};

// host: the row blocks of M rows on ncu CUs and the grid that runs them (knob "half_blocks", default 1 since
// measured: DeepFM B = 49,152 137-161 -> 180-182 M examples/s, profiles/r04/ab_round4_first.txt)
inline QRows q_rows(int M, int ncu, int& grid) {
  QRows r{M, 1, 0, 0};
  const int nb = (M + kQBM - 1) / kQBM;
  ncu = ncu > 0 ? ncu : 1;
  const int R = (nb + ncu - 1) / ncu, last = nb - (R - 1) * ncu;
  if (tuning_get("half_blocks", 1) != 0 && 2 * last <= ncu) {
    r.nfull = (R - 1) * ncu;
    r.nhalf = (M - r.nfull * kQBM + kQBM / 2 - 1) / (kQBM / 2);
    grid = r.nfull > 0 ? ncu : (r.nhalf < ncu ? r.nhalf : ncu);
  } else {
    r.nfull = nb;
    grid = nb < ncu ? nb : ncu;
  }
  r.G = grid;
  return r;
}

// host: whether the launch's (half) row blocks occupy every CU at least once
inline bool q_fills(int M, int ncu) {
  int grid = 0;
  (void)q_rows(M, ncu, grid);
  return grid >= ncu;
}

// unit start: this unit's DMAs (issued two units ago) have landed for this wave (N = vector-memory
// instructions the wave issued during the previous unit), then for every wave; the slot the next DMAs
// overwrite was read by every wave before this barrier
template <int N>
__device__ __forceinline__ void q_enter() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// the ReLU mask bits of a lane's outputs (training, k_layer_s3.hip): tile t's four outputs (n = 16 t + 4 g + q)
// at bits 4 t + q of the lane's 4-word group (100 of 128 bits for 25 tiles).  v is a ReLU output (> 0 or +0),
// so its bit is min(bits(v), 1): integer ops only (compares would hold 100 lane masks in SGPR pairs: the
// head spilled 179 SGPRs with them)
__device__ __forceinline__ void bits_set(uint32_t (&mb)[4], int t, const f32x4& v) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int i = 4 * t + q;
    mb[i >> 5] |= min(__float_as_uint(v[q]), 1u) << (i & 31);
  }
}

__device__ __forceinline__ f32x4 relu4(f32x4 v) {
#pragma unroll
  for (int r = 0; r < 4; ++r) v[r] = v[r] > 0.f ? v[r] : 0.f;
  return v;
}

// The output dot of a layer-3 column half HF (the tail's and the fused tower's layer 3): ReLU(acc + b3)[n] * wo[n]
// over n = 16 (13 HF + t) + 4 g + q (half 1 computes 12 tiles, tile 25 is padding), b3 and wo [416] in LDS,
// added into the row's partial logit.
template <int HF>
__device__ __forceinline__ void q_dot_half(const f32x4 (&acc)[kQUT], const float* b3, const float* wo, int g,
                                           float& part) {
  constexpr int NT = HF == 0 ? kQUT : kQNT - kQUT;
  __builtin_amdgcn_sched_barrier(0);  // (the epilogue's LDS reads hoisted into the last unit spilled)
  int g4 = 4 * g;
  asm volatile("" : "+v"(g4));  // (the 2 x 13 LDS addresses formed here, not hoisted into spills)
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int n0 = 16 * (kQUT * HF + t) + g4;
    const f32x4 bb = *reinterpret_cast<const f32x4*>(b3 + n0);
    const f32x4 wv = *reinterpret_cast<const f32x4*>(wo + n0);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float v = acc[t][r] + bb[r];
      v = v > 0.f ? v : 0.f;
      part += v * wv[r];
    }
  }
  // the dot is done here: sunk to its use after half 1, it kept half 0's 13 accumulators alive and spilled
  asm volatile("" : "+v"(part));
}

// ---- the stored-A stream (k_tail_s3.hip's h1, k_layer_s3.hip's A): A [M][lda] fp32 streams from HBM by LDS-DMA
// into two per-wave 2-KiB step slots (the wave's 16 rows x 128 B); only the issuing wave reads them: its own
// vmcnt orders them, no barrier.
constexpr int kQAKS = 13;              // 32-wide K steps of a 400-wide A (Kpad = 416)
constexpr int kQAWave = 2 * 2048;      // per wave: two step slots

// a zero A row: the load source of rows past M (every lane issues the same loads at every K offset); also a
// zero source of other loads that must be issued for rows past M (k_layer_s3.hip's mask bits)
static __device__ __attribute__((aligned(16))) float g_qzero_row[kQN];

// A of K step c of the row block at row0 (nw waves own rows) into this wave's slot ds (2 DMA instructions;
// rows past M read the zero row).  Instruction i, lane L: row r = 8 i + (L >> 3), physical 16-B slot L & 7,
// which holds logical slot j = (L & 7) ^ (r & 7), i.e. columns 32 c + 4 j .. + 3 (j < 4: the fragment's a0
// part, j >= 4: a1).
__device__ __forceinline__ void a_dma(const float* A, int lda, int M, const float* zrow, char* alds, int row0, int nw,
                                      int c, int ds, int w, int lane) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    int r = 8 * i + (lane >> 3), j = (lane & 7) ^ ((lane >> 3) & 7);
    asm volatile("" : "+v"(r), "+v"(j));  // formed here (not hoisted)
    // branch-free (an exec-masked address branch split the unit into basic blocks): rows past M
    // read the zero row at the same column offset (M * lda < 2^31: launch check)
    const int m = row0 + w * 16 + r;
    const uint32_t ok = (w < nw && m < M) ? 1u : 0u;
    const uintptr_t base = (uintptr_t)zrow + (uintptr_t)ok * ((uintptr_t)A - (uintptr_t)zrow);
    const float* row = reinterpret_cast<const float*>(base) + (uint32_t)(m * (int)ok) * (uint32_t)lda;
    lds_dma<16>(row + 32 * c + 4 * j, alds + ds * 2048 + i * 1024);
  }
}
// the A fragment of step c from the wave's slot c & 1: a0 = columns 32 c + 4 g .., a1 = 32 c + 16 + 4 g ..
// (zero at the last step: columns 400 .. are padding)
__device__ __forceinline__ void a_read(const char* alds, int c, int lane, f32x4& a0, f32x4& a1, int last_step) {
  const int r = lane & 15, g = lane >> 4;
  int o0 = r * 128 + ((g ^ (r & 7)) << 4), o1 = r * 128 + (((g + 4) ^ (r & 7)) << 4);
  asm volatile("" : "+v"(o0), "+v"(o1));
  a0 = *reinterpret_cast<const f32x4*>(alds + (c & 1) * 2048 + o0);
  a1 = *reinterpret_cast<const f32x4*>(alds + (c & 1) * 2048 + o1);
  if (c == last_step) a1 = f32x4{0.f, 0.f, 0.f, 0.f};
}

// ---- the gathered-A stream (DeepFM layer 1 in k_head_s3.hip and k_fused_s3.hip): per K step (two fields) a
// wave DMAs its 16 samples' two 64-B table rows into its own A slot, addressed by ids that were DMA'd into a
// small per-wave ring three steps earlier; the first-order weights ride a per-wave ring the same way.  The
// wave's steps s = 0, 1, ... run on over its row blocks: step s is K step s % KS of row block
// blockIdx.x + (s / KS) gridDim.x (none past the last); its ring slots are s & 3 (ids) and s & 1 (rows, weights).
constexpr int kGMaxF = 40;                       // fields (K = 16 F <= 640, 20 K steps)
constexpr int kGA = 2 * 2 * 16 * 64;             // per wave: 2 slots x [2 fields][16 samples][64 B]
constexpr int kGId = 4 * 128;                    // per wave: 4 slots x [2 fields][16] ids
constexpr int kGWr = 2 * 128;                    // per wave: 2 slots x [2 fields][16] first-order weights
constexpr int kGWave = kGA + kGId + kGWr;

// the stream's kernel arguments, embedded in HeadS3Args / FusedS3Args where these fields always sat (M and F
// stay at the head of those structs: the argument offsets do not move)
struct GatherArgs {
  const int32_t* ids;     // [M][F]
  const float* table;     // row of id at table + (id << gsh) (16 fp32: k = 16)
  int gsh;
  const float* wtab;      // first-order weight of id at wtab[id << wsh]
  int wsh;
};

// ids of K step c of the row block at row0 (nw waves own rows) into id slot `slot` (lanes 0 .. 31: field
// 2c + (L >> 4) of sample L & 15; past M or F, or for a wave without rows: -1)
__device__ __forceinline__ void g_id_dma(const int32_t* ids, int M, int F, char* wl, int row0, int nw, int c, int slot,
                                         int w, int lane) {
  int f = lane >> 4, r = lane & 15;
  asm volatile("" : "+v"(f), "+v"(r));
  const int m = row0 + w * 16 + r, fld = 2 * c + f;
  const bool ok = w < nw && m < M && fld < F;
  const int32_t* src = ok ? ids + (int64_t)m * F + fld : g_rmx_neg1;
  if (lane < 32)
    lds_dma<4>(src, wl + kGA + slot * 128);
}
// ... of the wave's step s
__device__ __forceinline__ void g_id_dma_step(const int32_t* ids, int M, int F, const QRows& rows, int KS, char* wl,
                                              int s, int w, int lane) {
  const int it = s / KS, c = s - it * KS;
  int row0, nw;
  rows.desc(blockIdx.x, it, row0, nw);
  g_id_dma(ids, M, F, wl, row0, nw, c, s & 3, w, lane);
}

// step s's three ids per lane (the rows of fields 2c, 2c + 1 and the weight), read from id slot s & 3.  A
// kernel whose row DMAs ride its MFMA stream reads them at the unit's head, beside its other LDS reads
// (k_fused_s3.hip: read at the DMA, each id needed an s_waitcnt lgkmcnt(0) that also drained the B fragments
// prefetched for the next tiles -- three times per half-0 unit).
struct GRowIds {
  int id0, id1, idw;
};
__device__ __forceinline__ GRowIds g_row_ids(char* wl, int s, int lane) {
  const int* ids = reinterpret_cast<const int*>(wl + kGA + (s & 3) * 128);
  int r = lane >> 2, lw = lane & 31;
  asm volatile("" : "+v"(r), "+v"(lw));
  return GRowIds{ids[r], ids[16 + r], ids[lw]};
}
// rows (2 DMAs: field f = instruction, lane L: sample L >> 2, physical 16-B slot L & 3 = logical slot
// swz_slot(sample, L & 3)) and first-order weights (lanes 0 .. 31) of the wave's step s into A slot s & 1 /
// weight slot s & 1.  part 0 / 1: the row of field 2c / 2c + 1; part 2: the weights
__device__ __forceinline__ void g_row_dma_ids(const GatherArgs& ga, char* wl, int s, int lane, const GRowIds& q,
                                              int part) {
  int g = swz_slot(lane >> 2, lane & 3);
  asm volatile("" : "+v"(g));
  const float* zero16 = g_rmx_zero16;
  char* a = wl + (s & 1) * 2048;
  if (part == 0) lds_dma<16>(q.id0 >= 0 ? ga.table + ((int64_t)q.id0 << ga.gsh) + 4 * g : zero16, a);
  if (part == 1) lds_dma<16>(q.id1 >= 0 ? ga.table + ((int64_t)q.id1 << ga.gsh) + 4 * g : zero16, a + 1024);
  if (part == 2 && lane < 32)
    lds_dma<4>(q.idw >= 0 ? ga.wtab + ((int64_t)q.idw << ga.wsh) : zero16, wl + kGA + kGId + (s & 1) * 128);
}
// all three, the ids read here, every address formed before the first DMA is issued: k_head_s3.hip, which
// issues them ahead of the unit's MFMAs.  (k_fused_s3.hip issues them inside its MFMA stream from ids in
// registers, g_row_dma_ids; for its prologue and its waves without rows it keeps a copy in its own order,
// f_row_dma there says why.)
__device__ __forceinline__ void g_row_dma(const GatherArgs& ga, char* wl, int s, int lane) {
  const int* ids = reinterpret_cast<const int*>(wl + kGA + (s & 3) * 128);
  int r = lane >> 2, g = swz_slot(lane >> 2, lane & 3), lw = lane & 31;
  asm volatile("" : "+v"(r), "+v"(g), "+v"(lw));
  const int id0 = ids[r], id1 = ids[16 + r], idw = ids[lw];
  const float* zero16 = g_rmx_zero16;
  const float* s0 = id0 >= 0 ? ga.table + ((int64_t)id0 << ga.gsh) + 4 * g : zero16;
  const float* s1 = id1 >= 0 ? ga.table + ((int64_t)id1 << ga.gsh) + 4 * g : zero16;
  const float* sw = idw >= 0 ? ga.wtab + ((int64_t)idw << ga.wsh) : zero16;
  char* a = wl + (s & 1) * 2048;
  lds_dma<16>(s0, a);
  lds_dma<16>(s1, a + 1024);
  if (lane < 32)
    lds_dma<4>(sw, wl + kGA + kGId + (s & 1) * 128);
}

// host: a row-owner kernel's auto knob -- 0 off, 2 always, 1 (default) when the (half) row blocks fill every
// CU at least once, or -- with half blocks -- at any batch above the whole-tower kernel's one round
// (k_small_s3.hip: M <= 16 ncu): half blocks on part of the chip still beat three engine launches
inline bool q_auto(const char* knob, int M) {
  const int v = tuning_get(knob, 1);
  if (v == 0) return false;
  if (v == 2) return true;
  const int ncu = cu_count_or(256);
  return q_fills(M, ncu) || (tuning_get("half_blocks", 1) != 0 && M > 16 * ncu);
}

}  // namespace rowown
}  // namespace rmx
