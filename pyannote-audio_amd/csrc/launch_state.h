// What a launch knows about its device -- the dynamic LDS its kernel may use there, the workgroups of a persistent
// kernel it holds, a few attributes -- belongs to a DEVICE and a KERNEL, not to the process or the call site: written
// down here once, in plain C++ without HIP (tests/native/launch_state_harness.cpp compiles it for the host).
#pragma once
#include <atomic>
#include <mutex>
namespace pa {
namespace devq {   // the device queries: pa_core.cpp defines them with HIP, the harness with stubs
enum Attr { CU_COUNT, LDS_PER_WORKGROUP, WALL_CLOCK_KHZ };
int current();                                                  // the calling thread's current device
long attribute(int dev, Attr which);                            // <= 0: the query failed
bool set_dynamic_lds(const void* kernel, long bytes);           // on the current device
int blocks_per_cu(const void* kernel, int threads, long lds);   // the occupancy API; <= 0: it failed
}  // namespace devq
// One positive value per device, 0 = none yet; a device outside the table is served from NO slot: it works uncached
constexpr int MAXDEV = 16;
inline std::mutex& grow_mutex() { static std::mutex m; return m; }   // the slow path of DeviceCell::raise, nothing else
class DeviceCell {
 public:
  static bool holds(int dev) { return dev >= 0 && dev < MAXDEV; }
  // fill() on first use, then one acquire load and no lock; racing threads both fill, with one value.  <= 0: not kept
  template <class Fill>
  long get(int dev, Fill fill) {
    if (!holds(dev)) return fill();
    long v = v_[dev].load(std::memory_order_acquire);
    if (v == 0 && (v = fill()) > 0) v_[dev].store(v, std::memory_order_release);
    return v;
  }
  // grow-only: set(want) runs only for a `want` above the grant so far; that slow path alone is serialised, so that
  // requests that differ cannot overtake each other between set() and the store
  template <class Set>
  bool raise(int dev, long want, Set set) {
    if (!holds(dev)) return set(want);
    if (want <= v_[dev].load(std::memory_order_acquire)) return true;
    std::lock_guard<std::mutex> lock(grow_mutex());
    if (want <= v_[dev].load(std::memory_order_relaxed)) return true;
    if (!set(want)) return false;
    v_[dev].store(want, std::memory_order_release);
    return true;
  }
 private:
  std::atomic<long> v_[MAXDEV] = {};
};
// the cell of one kernel: per FUNCTION -- kernels of one signature share a type (and so a generic lambda's statics)
template <auto Kernel> DeviceCell& kernel_cell() { static DeviceCell cell; return cell; }
// device attributes, asked once per device; `fallback` where the query fails
inline long device_attribute(devq::Attr which, int dev, long fallback) {
  static DeviceCell cells[3];
  const long v = cells[which].get(dev, [&] { return devq::attribute(dev, which); });
  return v > 0 ? v : fallback;
}
// "allow this kernel `bytes` of LDS on the current device" (`granted`: its kernel_cell); above the limit: refused unasked
enum LdsAnswer { LDS_OK = 0, LDS_OVER_LIMIT = 1, LDS_SET_FAILED = 2 };
inline long lds_limit(int dev) { return device_attribute(devq::LDS_PER_WORKGROUP, dev, 0); }   // 0: unknown, unchecked
inline LdsAnswer request_lds(int dev, const void* kernel, long bytes) {
  const long limit = lds_limit(dev);
  if (limit > 0 && bytes > limit) return LDS_OVER_LIMIT;
  return devq::set_dynamic_lds(kernel, bytes) ? LDS_OK : LDS_SET_FAILED;
}
inline LdsAnswer allow_lds(DeviceCell& granted, const void* kernel, long bytes) {
  const int dev = devq::current();
  LdsAnswer a = LDS_OK;
  granted.raise(dev, bytes, [&](long b) { return (a = request_lds(dev, kernel, b)) == LDS_OK; });
  return a;
}
// "how many workgroups of this kernel does the current device hold": CUs x `per_cu`, with PER_CU_ASK CUs x what the
// occupancy API answers (2 where it does not), after asking for the LDS it depends on.  <= 0: -LdsAnswer.
constexpr int PER_CU_ASK = 0;
inline long resident_workgroups(DeviceCell& cell, const void* kernel, int threads, long lds, int per_cu) {
  const int dev = devq::current();
  return cell.get(dev, [&]() -> long {
    const LdsAnswer a = request_lds(dev, kernel, lds);
    if (a != LDS_OK) return -(long)a;
    int n = per_cu;
    if (n == PER_CU_ASK && (n = devq::blocks_per_cu(kernel, threads, lds)) < 1) n = 2;
    return device_attribute(devq::CU_COUNT, dev, 256) * n;
  });
}
// grid of a persistent kernel: the resident workgroups in whole XCD stripes of 8, or one per tile (`halves`: per 2 tiles)
inline int persistent_grid(long total, long resident, bool halves = false) {
  const long whole = resident & ~7L, want = halves ? (total + 1) / 2 : total;
  return (int)(want < whole ? (halves ? (want + 7) & ~7L : want) : whole);
}
}  // namespace pa
