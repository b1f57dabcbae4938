// Caller-allocated workspaces: ONE function per entry point walks a pa::Carver and fills the kernel's state struct.
// Over a null base it is the sizing pass behind pa_*_workspace_bytes, over the caller's pointer it hands out the
// arrays, and the entry point refuses a workspace smaller than bytes() before anything is enqueued: size and carving
// are the same walk.  Plain C++ without HIP: tests/native/carver_harness.cpp compiles this header for the host.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace pa {

constexpr size_t align_up(size_t v, size_t align = 256) { return (v + align - 1) / align * align; }

class Carver {
 public:
  // `base` null: a sizing pass (its pointers are offsets from null and must not be used).  `slack` != 0: the caller's
  // pointer may be unaligned; the blocks start at its next multiple of `slack`, which bytes() counts in both passes.
  explicit Carver(void* base, size_t slack = 0)
      : base_(slack != 0 ? align_up((uintptr_t)base, slack) : (uintptr_t)base), slack_(slack) {}

  // `count` elements of T at the next multiple of `align`.  A block owns its bytes up to the next multiple of its OWN
  // alignment: align = 256 gives the block-aligned layouts, align = sizeof(T) arrays placed back to back.
  template <class T>
  T* take(size_t count, size_t align = 256) {
    off_ = align_up(align_up(off_, last_align_), align);
    T* p = reinterpret_cast<T*>(base_ + off_);
    off_ += count * sizeof(T);
    last_align_ = align;
    return p;
  }

  // what the blocks taken so far need, the last one rounded up like the others
  size_t bytes() const { return slack_ + align_up(off_, last_align_); }

 private:
  uintptr_t base_;
  size_t slack_, off_ = 0, last_align_ = 1;
};

// bytes() of the sizing pass of `layout(carver)`
template <class Layout>
size_t carved_bytes(Layout layout, size_t slack = 0) {
  Carver sizing(nullptr, slack);
  layout(sizing);
  return sizing.bytes();
}

}  // namespace pa
