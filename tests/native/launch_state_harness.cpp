// Host harness for csrc/launch_state.h: the per-device cell and the rules on top of it, compiled for the host (once
// with -fsanitize=address,undefined, once with -fsanitize=thread) against stubbed device queries that count what they
// are asked.  The "current device" of the stubs is a thread-local variable.
//   (a) eight threads on two devices: every caller reads its own device's value, the setup runs at least once per
//       device and only ever for the device asked
//   (b) the grow-only LDS rule: 66 KB, 132 KB, 66 KB on device 0, 66 KB on device 1 -> three set calls, 2 + 1
//   (c) device -1 and device MAXDEV are served from no slot: computed every time, no other device's value touched
//   (d) a request above the device's limit is refused before any set call
//   (e) the grid functions equal the literal expressions of the five persistent launchers
//   (f) kernels of ONE signature (one function-pointer type, as the four nn-chain kernels are) have a cell each: the
//       second one's request reaches the device although the first one's was granted
// usage: harness  ->  exit code 0 iff every check held (the first failure is printed).
#include <atomic>
#include <cstdio>
#include <thread>
#include <vector>

#include "launch_state.h"

static thread_local int t_dev = 0;
static const int FAKE_DEVS = pa::MAXDEV + 1;           // devices 0 .. MAXDEV; -1 counts at index FAKE_DEVS (slot())
static std::atomic<int> g_sets[FAKE_DEVS + 1], g_occ[FAKE_DEVS + 1], g_attr[FAKE_DEVS + 1];
static std::atomic<int> g_foreign{0};                  // queries that named another device than the caller's
static long g_limit = 160 * 1024;
static int slot(int dev) { return dev < 0 ? FAKE_DEVS : dev; }

namespace pa {
namespace devq {
int current() { return t_dev; }
long attribute(int dev, Attr which) {
  if (dev != t_dev) ++g_foreign;
  ++g_attr[slot(dev)];
  // device d: 8 (d + 2) CUs, the LDS limit of the test, 100 MHz
  return which == CU_COUNT ? 8 * (dev + 2) : which == LDS_PER_WORKGROUP ? g_limit : 100000;
}
bool set_dynamic_lds(const void*, long) {
  ++g_sets[slot(t_dev)];
  return true;
}
int blocks_per_cu(const void*, int, long) {
  ++g_occ[slot(t_dev)];
  return 2;
}
}  // namespace devq
}  // namespace pa

#define CHECK(cond, ...)          \
  do {                            \
    if (!(cond)) {                \
      fprintf(stderr, __VA_ARGS__); \
      fprintf(stderr, "\n");      \
      return false;               \
    }                             \
  } while (0)

static void reset_counts() {
  for (int i = 0; i <= FAKE_DEVS; ++i) g_sets[i] = g_occ[i] = g_attr[i] = 0;
  g_foreign = 0;
}
static const int KERNEL = 0;   // a kernel's address

static bool threads_on_two_devices() {
  reset_counts();
  static pa::DeviceCell cell;
  std::atomic<int> wrong{0};
  std::vector<std::thread> pool;
  for (int t = 0; t < 8; ++t)
    pool.emplace_back([&, t] {
      t_dev = t & 1;
      for (int i = 0; i < 20000; ++i) {
        const long got = pa::resident_workgroups(cell, &KERNEL, 256, 70000, pa::PER_CU_ASK);
        if (got != 8L * (t_dev + 2) * 2) ++wrong;
        if (pa::device_attribute(pa::devq::CU_COUNT, t_dev, 256) != 8L * (t_dev + 2)) ++wrong;
      }
    });
  for (auto& th : pool) th.join();
  CHECK(wrong == 0, "(a) %d calls read another value than their device's", wrong.load());
  CHECK(g_foreign == 0, "(a) %d queries named a device that was not the caller's", g_foreign.load());
  for (int d = 0; d < 2; ++d) {
    // at most once per thread of the device: a filled cell is not set up again
    CHECK(g_sets[d] >= 1 && g_sets[d] <= 4, "(a) device %d: LDS set %d times", d, g_sets[d].load());
    CHECK(g_occ[d] >= 1 && g_occ[d] <= 4, "(a) device %d: occupancy asked %d times", d, g_occ[d].load());
  }
  for (int d = 2; d <= FAKE_DEVS; ++d)
    CHECK(g_sets[d] == 0 && g_occ[d] == 0 && g_attr[d] == 0, "(a) device slot %d was set up and nobody asked", d);
  return true;
}

static bool grow_only() {
  reset_counts();
  pa::DeviceCell granted;
  const long kb66 = 66 * 1024 + 512, kb132 = 132 * 1024;
  t_dev = 0;
  CHECK(pa::allow_lds(granted, &KERNEL, kb66) == pa::LDS_OK && g_sets[0] == 1, "(b) first request: %d sets", g_sets[0].load());
  CHECK(pa::allow_lds(granted, &KERNEL, kb132) == pa::LDS_OK && g_sets[0] == 2, "(b) larger request: %d sets", g_sets[0].load());
  CHECK(pa::allow_lds(granted, &KERNEL, kb66) == pa::LDS_OK && g_sets[0] == 2, "(b) smaller request: %d sets", g_sets[0].load());
  t_dev = 1;
  CHECK(pa::allow_lds(granted, &KERNEL, kb66) == pa::LDS_OK && g_sets[1] == 1, "(b) device 1: %d sets", g_sets[1].load());
  CHECK(g_sets[0] == 2, "(b) device 1's request counted for device 0");
  int all = 0;
  for (int i = 0; i <= FAKE_DEVS; ++i) all += g_sets[i];
  CHECK(all == 3, "(b) %d set calls in all, 3 expected", all);
  return true;
}

static bool outside_the_table() {
  const int outside[2] = {-1, pa::MAXDEV};
  for (int dev : outside) {
    reset_counts();
    CHECK(!pa::DeviceCell::holds(dev), "(c) device %d counts as held", dev);
    pa::DeviceCell cell;
    // fill every slot of the table with a value no outside device may see
    for (int d = 0; d < pa::MAXDEV; ++d) cell.get(d, [] { return 777L; });
    int fills = 0;
    for (int i = 0; i < 3; ++i) {
      const long v = cell.get(dev, [&] { ++fills; return 5L; });
      CHECK(v == 5, "(c) device %d read %ld from a slot", dev, v);
    }
    CHECK(fills == 3, "(c) device %d: computed %d times in 3 calls", dev, fills);
    for (int d = 0; d < pa::MAXDEV; ++d) CHECK(cell.get(d, [] { return -1L; }) == 777, "(c) slot %d was overwritten", d);
    // the same through the two rules: every call asks the device
    pa::DeviceCell granted, resident;
    t_dev = 0;
    CHECK(pa::allow_lds(granted, &KERNEL, 100000) == pa::LDS_OK, "(c) device 0 refused");
    pa::resident_workgroups(resident, &KERNEL, 256, 100000, 1);
    reset_counts();
    t_dev = dev;
    for (int i = 0; i < 3; ++i) {
      CHECK(pa::allow_lds(granted, &KERNEL, 100000) == pa::LDS_OK, "(c) device %d refused", dev);
      CHECK(pa::resident_workgroups(resident, &KERNEL, 256, 100000, 1) == 8L * (dev + 2),
            "(c) device %d was answered with another device's workgroups", dev);
    }
    CHECK(g_sets[slot(dev)] == 6 && g_sets[0] == 0, "(c) device %d: %d set calls in 3 + 3 requests", dev, g_sets[slot(dev)].load());
    CHECK(g_foreign == 0, "(c) a query named another device");
  }
  return true;
}

static bool over_the_limit() {
  reset_counts();
  g_limit = 64 * 1024;
  t_dev = 3;   // (a device no other check uses: its limit is remembered)
  pa::DeviceCell granted, resident;
  const pa::LdsAnswer a = pa::allow_lds(granted, &KERNEL, 64 * 1024 + 1);
  const long r = pa::resident_workgroups(resident, &KERNEL, 256, 64 * 1024 + 1, 1);
  const pa::LdsAnswer fits = pa::allow_lds(granted, &KERNEL, 64 * 1024);
  g_limit = 160 * 1024;
  CHECK(a == pa::LDS_OVER_LIMIT, "(d) a request above the limit was answered %d", (int)a);
  CHECK(r == -(long)pa::LDS_OVER_LIMIT, "(d) a persistent kernel above the limit was given %ld workgroups", r);
  CHECK(fits == pa::LDS_OK && g_sets[3] == 1, "(d) %d set calls, 1 (the request at the limit) expected", g_sets[3].load());
  return true;
}

static bool grid_rule() {
  const int cus[] = {8, 64, 256, 304}, per_cu[] = {1, 2};
  const long totals[] = {1, 7, 8, 9, 511, 512, 513, 1000000};
  for (int c : cus)
    for (int p : per_cu)
      for (long total : totals) {
        // the launchers' own lines: an int table entry, `& ~7`, min; k_conv3x3_wino32's halving
        const int resident_of = c * p;
        const int resident = resident_of & ~7;
        const int grid = (int)(total < resident ? total : resident);
        const long want = (total + 1) / 2;
        const int grid32 = (int)(want < resident ? ((want + 7) & ~7L) : resident);
        CHECK(pa::persistent_grid(total, resident_of) == grid, "(e) cus %d x %d, total %ld: grid %d, launcher %d", c, p,
              total, pa::persistent_grid(total, resident_of), grid);
        CHECK(pa::persistent_grid(total, resident_of, true) == grid32, "(e) cus %d x %d, total %ld: halves %d, launcher %d",
              c, p, total, pa::persistent_grid(total, resident_of, true), grid32);
      }
  return true;
}

template <int METHOD>
static void fake_kernel(double*, int) {}

static bool cell_per_kernel() {
  reset_counts();
  t_dev = 0;
  auto ask = [](auto kernel_of_one_type, pa::DeviceCell& cell) {   // (instantiated once for all three kernels)
    return pa::allow_lds(cell, reinterpret_cast<const void*>(kernel_of_one_type), 100000);
  };
  for (int round = 0; round < 2; ++round) {
    CHECK(ask(fake_kernel<0>, pa::kernel_cell<fake_kernel<0>>()) == pa::LDS_OK, "(f) kernel 0 refused");
    CHECK(ask(fake_kernel<1>, pa::kernel_cell<fake_kernel<1>>()) == pa::LDS_OK, "(f) kernel 1 refused");
    CHECK(ask(fake_kernel<2>, pa::kernel_cell<fake_kernel<2>>()) == pa::LDS_OK, "(f) kernel 2 refused");
    CHECK(g_sets[0] == 3, "(f) round %d: %d set calls for three kernels of one signature, 3 expected", round, g_sets[0].load());
  }
  CHECK(&pa::kernel_cell<fake_kernel<0>>() != &pa::kernel_cell<fake_kernel<1>>(), "(f) two kernels share a cell");
  return true;
}

int main() {
  if (!threads_on_two_devices() || !grow_only() || !outside_the_table() || !over_the_limit() || !grid_rule() ||
      !cell_per_kernel())
    return 1;
  printf("launch state held\n");
  return 0;
}
