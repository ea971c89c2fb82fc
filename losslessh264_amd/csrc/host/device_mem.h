// device_mem.h - what the host side of every pipeline needs of the HIP runtime, once: buffers that grow or are reused, one object
// per device behind a lock, the clock and the switch of the trace lines.  Header only; included by the .hip files (not by the host
// front end, which never sees the runtime).
#pragma once
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <chrono>
#include <memory>
#include <mutex>

namespace lh264host {

// device memory, grown (to bytes + bytes / 8) when a call needs more, reused otherwise.  Growing frees the old block first, which
// synchronises the device: nobody reads the old one any more.
struct DevBuf {
  void* p = nullptr; size_t cap = 0;
  hipError_t err = hipSuccess;            // what the last alloc() that failed got from the runtime
  DevBuf() = default;
  DevBuf (const DevBuf&) = delete;
  DevBuf& operator= (const DevBuf&) = delete;
  ~DevBuf() { if (p) (void)hipFree (p); }
  bool alloc (size_t bytes) {
    if (bytes < 16) bytes = 16;
    if (bytes <= cap) return true;
    if (p) { (void)hipFree (p); p = nullptr; cap = 0; }
    const size_t want = bytes + bytes / 8;
    if ((err = hipMalloc (&p, want)) != hipSuccess) { p = nullptr; return false; }
    cap = want;
    return true;
  }
  bool zero (size_t bytes, hipStream_t st) { return hipMemsetAsync (p, 0, bytes < 16 ? 16 : bytes, st) == hipSuccess; }
  template <typename T> T* as() const { return (T*)p; }
};
// page-locked staging memory (copies run at PCIe speed and asynchronously), same policy
struct PinBuf {
  void* p = nullptr; size_t cap = 0;
  hipError_t err = hipSuccess;
  PinBuf() = default;
  PinBuf (const PinBuf&) = delete;
  PinBuf& operator= (const PinBuf&) = delete;
  ~PinBuf() { if (p) (void)hipHostFree (p); }
  bool alloc (size_t bytes) {
    if (bytes < 16) bytes = 16;
    if (bytes <= cap) return true;
    if (p) { (void)hipHostFree (p); p = nullptr; cap = 0; }
    const size_t want = bytes + bytes / 8;
    if ((err = hipHostMalloc (&p, want, hipHostMallocDefault)) != hipSuccess) { p = nullptr; return false; }
    cap = want;
    return true;
  }
  template <typename T> T* as() const { return (T*)p; }
};

enum { kMaxDevices = 16 };

// One T per device, created when first asked for, each behind its own lock: what a pipeline keeps between calls (arenas, work
// spaces).  One call at a time per device holds the lock; calls on different devices do not meet.
template <typename T> class PerDevice {
  struct Slot { std::mutex mu; std::unique_ptr<T> obj; };
  Slot slot_[kMaxDevices];
 public:
  // the lock of one device's slot, held while the Ref lives
  class Ref {
    std::unique_lock<std::mutex> lock_; Slot* s_;
   public:
    explicit Ref (Slot& s) : lock_ (s.mu), s_ (&s) {}
    T* peek() const { return s_->obj.get(); }                                        // nullptr: nothing was kept on this device
    T& get() const { if (!s_->obj) s_->obj.reset (new T()); return *s_->obj; }
  };
  // the current device's index; -1: none, or beyond kMaxDevices
  static int current() { int d = 0; return hipGetDevice (&d) == hipSuccess && d >= 0 && d < kMaxDevices ? d : -1; }
  Ref lock (int device) { return Ref (slot_[device]); }
  // f (the current device's T) under its lock, 0 where there is none (the *_arena_bytes calls); false: no current device
  template <typename F> bool read_current (F&& f) {
    const int d = current();
    if (d < 0) return false;
    Ref r (slot_[d]);
    f (r.peek());
    return true;
  }
  // every device's T is destroyed with its device current; the caller's device is current again afterwards
  void release_all() {
    int cur = 0;
    (void)hipGetDevice (&cur);
    for (int d = 0; d < kMaxDevices; d++) {
      std::lock_guard<std::mutex> lock (slot_[d].mu);
      if (slot_[d].obj) { (void)hipSetDevice (d); slot_[d].obj.reset(); }
    }
    (void)hipSetDevice (cur);
  }
};

inline double now_s() { return std::chrono::duration<double> (std::chrono::steady_clock::now().time_since_epoch()).count(); }
// LH264_TRACE_COMPRESS / _DECODE / _RESTORE: a line per stage on stderr (each caller keeps the answer in a static of its own)
inline bool trace_on (const char* env_name) { return getenv (env_name) != nullptr; }

}  // namespace lh264host
