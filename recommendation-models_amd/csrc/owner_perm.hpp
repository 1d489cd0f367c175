// owner_perm.hpp -- the keyed owner permutation of a sharded table (shard.hip, param_io.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

namespace rmx {

// The keyed permutation p of [0, V) (OwnerPerm.key == 0: identity): a 4-round Feistel network on
// the square domain Z_a x Z_a, a = ceil(sqrt(V)) (x = L a + R), each round (L, R) -> (R, (L + F_r(R))
// mod a) with F_r(R) = mulhi(fmix32(R ^ k_r), a) (the murmur3 finaliser; k_r four 32-bit round keys
// drawn from the key by splitmix64).  Cycle-walked back into [0, V): the domain exceeds V by < 2a,
// so a walk is rare (none at V = a^2, e.g. V = 10^8); every cycle re-enters [0, V) only if it started
// there.  All 32-bit integer work, ~40 instructions per id.
struct OwnerPerm {
  uint64_t key = 0;
  uint32_t a = 1;
  uint32_t rk[4] = {0, 0, 0, 0};
  int64_t V = 0;
};
__device__ __host__ __forceinline__ uint32_t owner_round(uint32_t x, uint32_t rk, uint32_t a) {
  uint32_t h = x ^ rk;
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return (uint32_t)(((uint64_t)h * a) >> 32);  // uniform in [0, a)
}
__device__ __host__ __forceinline__ uint32_t feistel_once(uint32_t x, const OwnerPerm& op, bool inverse) {
  const uint32_t a = op.a;
  uint32_t L = x / a, R = x - L * a;
  if (!inverse) {
    for (int r = 0; r < 4; ++r) {
      const uint32_t t = owner_round(R, op.rk[r], a);
      const uint32_t s = L + t;
      L = R;
      R = s >= a ? s - a : s;
    }
  } else {
    for (int r = 3; r >= 0; --r) {
      const uint32_t t = owner_round(L, op.rk[r], a);
      const uint32_t l = R >= t ? R - t : R + a - t;
      R = L;
      L = l;
    }
  }
  return L * a + R;
}
__device__ __host__ __forceinline__ int64_t owner_perm(int64_t id, const OwnerPerm& op, bool inverse) {
  if (!op.key) return id;
  uint32_t y = feistel_once((uint32_t)id, op, inverse);
  while ((int64_t)y >= op.V) y = feistel_once(y, op, inverse);
  return y;
}

inline OwnerPerm owner_perm_of(uint64_t key, int64_t V) {
  OwnerPerm op;
  op.key = key;
  op.V = V;
  uint64_t a = (uint64_t)std::sqrt((double)std::max<int64_t>(V, 1));
  while ((int64_t)(a * a) < V) ++a;
  while (a > 1 && (int64_t)((a - 1) * (a - 1)) >= V) --a;
  op.a = (uint32_t)a;
  uint64_t z = key;
  for (int r = 0; r < 4; ++r) {  // round keys: splitmix64 of the key, successive states
    z += 0x9E3779B97F4A7C15ULL;
    uint64_t x = z;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ULL;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBULL;
    op.rk[r] = (uint32_t)(x ^ (x >> 31));
  }
  return op;
}

}  // namespace rmx
