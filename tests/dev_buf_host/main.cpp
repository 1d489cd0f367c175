// Host check of csrc/dev_buf.hpp: DevBuf / ScratchBuf over malloc-backed dev_raw_alloc / dev_raw_free, no GPU
// runtime.  Built with -fsanitize=address,undefined and run by tests/test_dev_buf_host.py: a double free, a leak
// or a use after a move ends the program with the sanitizer's report; a failed CHECK prints its line and exits 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "dev_buf.hpp"

static int64_t g_bytes = 0, g_buffers = 0;
static std::string g_err;

namespace rmx {
void set_error(const std::string& msg) { g_err = msg; }
void* dev_raw_alloc(size_t bytes) {
  if (bytes > (size_t(1) << 40)) return nullptr;  // "out of memory" without asking malloc for it
  g_bytes += (int64_t)bytes;
  ++g_buffers;
  return std::malloc(bytes);
}
void dev_raw_free(void* p, size_t bytes) {
  g_bytes -= (int64_t)bytes;
  --g_buffers;
  std::free(p);
}
}  // namespace rmx

using rmx::DevBuf;
using rmx::Scratch;
using rmx::ScratchBuf;

#define CHECK(cond)                                                \
  do {                                                             \
    if (!(cond)) {                                                 \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond);        \
      return 1;                                                    \
    }                                                              \
  } while (0)

static_assert(!std::is_copy_constructible<DevBuf<float>>::value && !std::is_copy_assignable<DevBuf<float>>::value, "");
static_assert(!std::is_copy_constructible<ScratchBuf<float>>::value, "");
static_assert(std::is_nothrow_move_constructible<DevBuf<float>>::value, "");
static_assert(std::is_nothrow_move_assignable<DevBuf<float>>::value, "");
static_assert(std::is_nothrow_move_constructible<ScratchBuf<float>>::value, "");
static_assert(std::is_nothrow_move_assignable<ScratchBuf<float>>::value, "");

// every registry entry is one of the buffers, with its size, and every allocated buffer has an entry
static bool registry_matches(const std::vector<Scratch>& reg, const std::vector<ScratchBuf<float>>& v) {
  size_t live = 0;
  for (const auto& b : v) {
    if (!b) continue;
    ++live;
    size_t hits = 0;
    for (const auto& e : reg) hits += e.ptr == b.get() && e.bytes == b.bytes();
    if (hits != 1) return false;
  }
  return live == reg.size();
}

static int run() {
  {  // alloc, min_n, read access
    DevBuf<float> a;
    CHECK(!a && a.get() == nullptr && a.bytes() == 0);
    CHECK(a.alloc(10, "t") == RMX_OK && a && a.bytes() == 40 && g_bytes == 40 && g_buffers == 1);
    float* raw = a;  // implicit read access
    CHECK(raw == a.get());
    raw[9] = 1.f;  // the whole size is there (the sanitizer checks)
    DevBuf<uint32_t> z, z4;
    CHECK(z.alloc(0, "t") == RMX_OK && z.bytes() == 4);        // default minimum: one element
    CHECK(z4.alloc(0, "t", 4) == RMX_OK && z4.bytes() == 16);  // min_n
    CHECK(z4.alloc(9, "t", 4) == RMX_OK && z4.bytes() == 36 && g_buffers == 3);
    DevBuf<void> v;
    CHECK(v.alloc(7, "t") == RMX_OK && v.bytes() == 7);  // bytes
    // alloc over a live buffer: the old one is freed
    CHECK(a.alloc(3, "t") == RMX_OK && a.bytes() == 12 && g_buffers == 4 && g_bytes == 12 + 4 + 36 + 7);
    // failure: empty, error text, nothing counted
    CHECK(a.alloc(size_t(1) << 41, "who") == RMX_E_NOMEM && !a && a.bytes() == 0 && g_buffers == 3);
    CHECK(g_err == "who: out of device memory (" + std::to_string((size_t(1) << 41) * 4) + " bytes)");
  }
  CHECK(g_bytes == 0 && g_buffers == 0);
  {  // moves
    DevBuf<float> a, b;
    CHECK(a.alloc(5, "t") == RMX_OK && b.alloc(6, "t") == RMX_OK);
    float* pa = a.get();
    DevBuf<float> c(std::move(a));  // construction: source empty, destination owns
    CHECK(!a && a.bytes() == 0 && c.get() == pa && c.bytes() == 20 && g_buffers == 2);
    b = std::move(c);  // assignment: old destination freed
    CHECK(!c && b.get() == pa && b.bytes() == 20 && g_buffers == 1 && g_bytes == 20);
    DevBuf<float>& self = b;
    b = std::move(self);  // self-move: untouched
    CHECK(b.get() == pa && b.bytes() == 20 && g_buffers == 1);
    b.reset();
    CHECK(!b && g_buffers == 0);
    b.reset();  // twice
  }
  CHECK(g_bytes == 0 && g_buffers == 0);
  {  // the registry
    std::vector<Scratch> reg;
    {
      ScratchBuf<float> s;
      CHECK(s.alloc(reg, 0, "t") == RMX_OK && reg.size() == 1 && reg[0].ptr == s.get() && reg[0].bytes == 4);
      CHECK(s.alloc(reg, 8, "t") == RMX_OK && reg.size() == 1 && reg[0].ptr == s.get() && reg[0].bytes == 32);
      ScratchBuf<float> t(std::move(s));
      CHECK(!s && reg.size() == 1 && reg[0].ptr == t.get());
      s.reset();  // the moved-from buffer owns no entry
      CHECK(reg.size() == 1);
      ScratchBuf<float> u;
      CHECK(u.alloc(reg, 2, "t") == RMX_OK && reg.size() == 2);
      u = std::move(t);  // u's old buffer and entry go, t's stay under u
      CHECK(!t && reg.size() == 1 && reg[0].ptr == u.get() && reg[0].bytes == 32 && g_buffers == 1);
      ScratchBuf<float>& self = u;
      u = std::move(self);
      CHECK(reg.size() == 1 && reg[0].ptr == u.get() && g_buffers == 1);
      CHECK(u.alloc(reg, size_t(1) << 41, "t") == RMX_E_NOMEM && !u && reg.empty() && g_buffers == 0);
    }
    CHECK(reg.empty());
    {  // a vector of registered buffers growing past its capacity (what TrainState's h / hm / u do)
      std::vector<ScratchBuf<float>> v;
      v.reserve(1);
      for (int i = 0; i < 9; ++i) {
        v.emplace_back();
        if (i % 3 != 2) CHECK(v.back().alloc(reg, (size_t)i + 1, "t") == RMX_OK);  // (some stay empty, like hm)
        CHECK(registry_matches(reg, v));
      }
      CHECK(reg.size() == 6 && g_buffers == 6);
      v.erase(v.begin() + 3);  // elements move down
      CHECK(registry_matches(reg, v) && reg.size() == 5);
      std::vector<ScratchBuf<float>> w(std::move(v));
      CHECK(registry_matches(reg, w) && reg.size() == 5);
      w = std::vector<ScratchBuf<float>>();  // the owner's "drop everything"
      CHECK(reg.empty() && g_buffers == 0);
    }
  }
  CHECK(g_bytes == 0 && g_buffers == 0);
  return 0;
}

int main() {
  const int rc = run();
  if (rc == 0) std::printf("dev_buf ok\n");
  return rc;
}
