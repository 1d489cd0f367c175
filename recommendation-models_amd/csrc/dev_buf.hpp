// dev_buf.hpp -- the owning device buffer of librmx.  Every device allocation of the library is a DevBuf (or a
// ScratchBuf) member of the object that owns it, so "what this object owns" is its member list and nothing
// else: dropping a buffer is reset() or the owner's destructor, on every path.
//
// Two orderings are the owner's to keep, a destructor cannot know them:
//  - hipDeviceSynchronize() (or the stream's) before a buffer that queued work may still read is reset;
//  - no DevBuf with static or thread storage duration: device memory is never freed while the process exits
//    (rmx.shutdown(), tests/test_teardown.py).  Owners are heap objects destroyed through the C ABI.
#pragma once

#include <cstddef>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/rmx.h"

namespace rmx {

void set_error(const std::string& msg);

// hipMalloc / hipFree and the live bytes / live buffers counters behind rmx_debug_live_device_memory
// (capi.hip; tests/dev_buf_host/main.cpp links malloc-backed ones).  bytes: what dev_raw_alloc was given.
void* dev_raw_alloc(size_t bytes);  // nullptr: out of memory
void dev_raw_free(void* p, size_t bytes);

template <class T>
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p_(o.p_), bytes_(o.bytes_) {
    o.p_ = nullptr;
    o.bytes_ = 0;
  }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      reset();
      std::swap(p_, o.p_);
      std::swap(bytes_, o.bytes_);
    }
    return *this;
  }
  ~DevBuf() { reset(); }

  // max(n, min_n) elements (bytes for DevBuf<void>), whatever the buffer held dropped first; on failure the
  // buffer is empty
  int alloc(size_t n, const char* who, size_t min_n = 1) {
    reset();
    const size_t bytes = kElem * (n > min_n ? n : min_n);
    if (!(p_ = static_cast<T*>(dev_raw_alloc(bytes)))) {
      set_error(std::string(who) + ": out of device memory (" + std::to_string(bytes) + " bytes)");
      return RMX_E_NOMEM;
    }
    bytes_ = bytes;
    return RMX_OK;
  }
  void reset() {
    if (p_) dev_raw_free(p_, bytes_);
    p_ = nullptr;
    bytes_ = 0;
  }

  T* get() const { return p_; }
  size_t bytes() const { return bytes_; }
  explicit operator bool() const { return p_ != nullptr; }
  operator T*() const { return p_; }

 private:
  static constexpr size_t kElem = sizeof(std::conditional_t<std::is_void<T>::value, char, T>);
  T* p_ = nullptr;
  size_t bytes_ = 0;
};

// What rmx_debug_poison_workspace fills: every live ScratchBuf of a model (rmx_model::scratch), with its
// allocated size.
struct Scratch {
  void* ptr;
  size_t bytes;
};

// A DevBuf listed in a scratch registry while it is allocated: a member of this type is floating-point scratch
// that rmx_debug_poison_workspace covers.  The registry must outlive the buffer.
template <class T>
class ScratchBuf : public DevBuf<T> {
 public:
  ScratchBuf() = default;
  ScratchBuf(ScratchBuf&& o) noexcept : DevBuf<T>(std::move(o)), reg_(o.reg_) { o.reg_ = nullptr; }
  ScratchBuf& operator=(ScratchBuf&& o) noexcept {
    if (this != &o) {
      reset();
      DevBuf<T>::operator=(std::move(o));
      std::swap(reg_, o.reg_);
    }
    return *this;
  }
  ~ScratchBuf() { reset(); }

  int alloc(std::vector<Scratch>& reg, size_t n, const char* who, size_t min_n = 1) {
    reset();
    const int st = DevBuf<T>::alloc(n, who, min_n);
    if (st == RMX_OK) {
      reg.push_back({this->get(), this->bytes()});
      reg_ = &reg;
    }
    return st;
  }
  void reset() {
    if (reg_)
      for (size_t i = 0; i < reg_->size(); ++i)
        if ((*reg_)[i].ptr == this->get()) {
          reg_->erase(reg_->begin() + i);
          break;
        }
    reg_ = nullptr;
    DevBuf<T>::reset();
  }

 private:
  std::vector<Scratch>* reg_ = nullptr;  // the entry is found by pointer: moving the buffer leaves it valid
};

}  // namespace rmx
