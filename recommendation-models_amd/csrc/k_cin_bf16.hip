// k_cin_bf16.hip -- the xDeepFM CIN on bf16 operands (rmx_model_set_cin_precision(RMX_DTYPE_BF16)), gfx950.
//
// The semantics are those of k_gemm.hip's CIN layer (CINEncoder.scala:36-58, 105-176); the arithmetic of the K
// reduction has exactly two storage points (include/rmx.h):
//   weights   C_l rounded to bf16 (RNE) element by element as given in mats, when the mats are packed;
//   operand   z[r][f * Hp + h] = bf16_rne(fl32(x0[r][f] * u_{l-1}[r][h])), in registers (k_gemm.hpp cin_a_bf16).
// One v_mfma_f32_16x16x32_bf16 per (row tile, column tile) per 32-wide K step, fp32 accumulation; bias, ReLU,
// the stored u_l and the rowdot epilogue (kEpiCin) are the fp32 CIN's, unchanged.
//
// K order: h-chunks hc of 16 maps, inside one the fields f (chunk c16 = hc * F + f), over every ordered pair --
// no layer-1 triangle fold (a folded weight C[f,h] + C[h,f] would be rounded after the sum).  A last h-chunk
// with <= 8 live maps carries two fields per chunk (k_gemm.hpp cin_chunk, cin_pair_hc): pure layout, the
// dropped positions are zeros.
#include "k_gemm.hpp"

namespace rmx {

// 16-wide chunks of a bf16 CIN layer's K order, and its paired h-chunk (-1: none)
int cin_bf16_chunks(int F, int Hp, int* pair_hc) {
  const int nhc = (Hp + 15) / 16;
  const bool pair = Hp - 16 * (nhc - 1) <= 8;
  if (pair_hc) *pair_hc = pair ? nhc - 1 : -1;
  return pair ? (nhc - 1) * F + (F + 1) / 2 : nhc * F;
}

int64_t cin_bf16_elems(int F, int Hp, int Npad) {
  return (int64_t)((cin_bf16_chunks(F, Hp, nullptr) + 1) / 2) * Npad * 32;
}

// C_l (H x F*Hp row-major, column f*Hp + h) -> [steps][Npad][32] bf16, each element rounded once (RNE).
// Position 8g + 4h + q of a 32-wide step holds lane group g's K value q of chunk 2s + h (plain chunk:
// z[j][16 hc + 4g + q]; paired: z[2j + g / 2][16 hc + 4 (g % 2) + q]) -- pack_split3_kernel's indexing
// with the hi plane alone.
__global__ void pack_cin_bf16_kernel(const float* __restrict__ C, int F, int Hp, int H, int Npad, int ncm,
                                     int pair_hc, int64_t tot, bf16_t* __restrict__ W16) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= tot) return;
  const int pos = (int)(i & 31);
  const int64_t rest = i >> 5;
  const int n = (int)(rest % Npad);
  const int s = (int)(rest / Npad);
  const int g = pos >> 3, h = (pos >> 2) & 1, q = pos & 3;
  const int c = 2 * s + h;
  float v = 0.f;
  if (c < ncm && n < H) {
    const int hc = c / F, j = c - hc * F;
    const bool pr = hc == pair_hc;
    const int f = pr ? 2 * j + (g >> 1) : j;
    const int hh = 16 * hc + (pr ? (g & 1) * 4 : g * 4) + q;
    if (f < F && hh < Hp) v = C[(int64_t)n * F * Hp + (int64_t)f * Hp + hh];
  }
  W16[i] = (bf16_t)v;
}

int launch_pack_cin_bf16(hipStream_t s, const float* mats, int F, CinLayer& L) {
  int pair_hc;
  const int ncm = cin_bf16_chunks(F, L.Hp, &pair_hc);
  const int64_t tot = cin_bf16_elems(F, L.Hp, L.Npad);
  hipLaunchKernelGGL(pack_cin_bf16_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, mats + L.w_off, F,
                     L.Hp, L.H, L.Npad, ncm, pair_hc, tot, L.W16.get());
  RMX_HIP(hipGetLastError());
  return RMX_OK;
}

// Npad == 208 (H in 193..208): the weight plane of a K step (13 KiB, 16 KiB with the padding that gives every
// wave whole DMA instructions) streams through a 3-deep LDS-DMA ring, the branch-free ring of the bf16 tower.
// A B fragment costs one ds_read_b128 per wave whatever MT is, and eight MT = 1 waves saturate the CU's LDS
// array, so the full tile is MT = 2: 32 rows per wave, in 4-wave blocks of 128 rows whose 74 KiB
// (ring + x0 tile at F = 39) let two share a CU -- one block's barrier and DMA wait meet the other's MFMAs
// (CIN 200^3 at B = 65,536, layer 2: 3.564 ms against 3.711 for one 8-wave block per CU, 3.845 / 3.667 for that
// block on a 2- / 4-deep ring; profiles/cin_bf16/ab_tiles.txt; the losers are not kept).  Below 256 rows per CU
// the rows go to more, smaller blocks (MT = 1, 4 or 2 waves: at most half the LDS array's rate per CU), as the
// fp32 CIN does (launch_cin_s3, knob-free here).  Same products in the same K order on every tile.
static int launch_cin_bf16_208(hipStream_t s, GemmArgs& p) {
  const int ncu = cu_count_or(256);
  auto blocks = [&](int rows) { return (int64_t)(p.M + rows - 1) / rows; };
  if (blocks(256) >= ncu) return launch_cfg<Tile<2, 13, 4, 1, 1, 2, 3, 0, 1>, kCinOuter, kEpiCin, kPrecBF16>(s, p);
  if (blocks(64) >= ncu) return launch_cfg<Tile<1, 13, 4, 1, 1, 2, 3, 0, 1>, kCinOuter, kEpiCin, kPrecBF16>(s, p);
  return launch_cfg<Tile<1, 13, 2, 1, 1, 2, 3, 0, 1>, kCinOuter, kEpiCin, kPrecBF16>(s, p);
}

// Every other width: a plain register-staged double buffer (the weight plane of a step is at most 16 KiB),
// 4 waves x 16 rows below M = 8,192 and 8 waves x 32 rows from there, the fp32 CIN's batch threshold.
template <int NT>
static int launch_cin_bf16_nt(hipStream_t s, GemmArgs& p) {
  if (p.M < 8192) return launch_cfg<Tile<1, NT, 4, 1, 1, 1>, kCinOuter, kEpiCin, kPrecBF16>(s, p);
  return launch_cfg<Tile<2, NT, 8, 1, 1, 1>, kCinOuter, kEpiCin, kPrecBF16>(s, p);
}

int launch_cin_layer_bf16(hipStream_t s, const CinLayer& L, bool first, bool last, int B, int F, int k,
                          const int32_t* ids, const float* table, const float* u_prev, float* u_out, float* rowdot,
                          int ld) {
  if (B <= 0) return RMX_OK;
  if (!L.W16) {
    set_error("cin: no bf16 weight plane (rmx_model_set_cin_precision, then rmx_model_set_mats)");
    return RMX_E_INVALID;
  }
  if (!first && !u_prev) {
    set_error("cin: missing previous layer maps");
    return RMX_E_INVALID;
  }
  GemmArgs p{};
  p.M = B * k;
  p.K = cin_bf16_chunks(F, L.Hp, &p.cin_pair_hc) * 16;
  p.Kpad = round_up(p.K, 32);
  p.Npad = L.Npad;
  p.ga = AGatherArgs{ids, table, F, k, ld > 0 ? ld : k};
  p.u_prev = u_prev;
  p.ldu = L.Hp_pad;
  p.XS = round_up(std::max(F, first ? L.Hp_pad : 0), 16) + 4;  // 16-B rows; x0 and (layer 1) u
  p.cin_first = first ? 1 : 0;
  p.Wp = reinterpret_cast<const float*>(L.W16.get());
  p.bias = L.b;
  p.C = last ? nullptr : u_out;
  p.ldc = L.Npad;
  p.wo = L.wo;
  p.rowdot = rowdot;
  if (p.K / 16 + 8 >= 65536 || F >= 65536) {  // the kernel's exact c16 / F (k_gemm.hpp div_f)
    set_error("cin: F * H_prev must stay below 1,048,448");
    return RMX_E_INVALID;
  }
  if (first && L.Hp_pad > p.XS - 4) {
    set_error("cin: first layer Hp_pad mismatch");
    return RMX_E_INVALID;
  }
  if (L.Npad == kS3BN) return launch_cin_bf16_208(s, p);
  switch (L.Npad / 16) {
#define RMX_NT(n) \
  case n: return launch_cin_bf16_nt<n>(s, p);
    RMX_NT(1) RMX_NT(2) RMX_NT(3) RMX_NT(4) RMX_NT(5) RMX_NT(6) RMX_NT(7)
    RMX_NT(8) RMX_NT(10) RMX_NT(16)
#undef RMX_NT
    default:
      set_error("cin: layer width must be <= 256");
      return RMX_E_INVALID;
  }
}

}  // namespace rmx
