// One table per kernel template: every compiled instantiation is one row, and launch, LDS attribute setup and "does this variant exist?"
// all read the same rows.  A kernel file builds its table with a short row macro, computes a key from the launch arguments and looks it up;
// a key with no row is refused.  Adding a variant = adding a row.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ns2vc {

// a row's key: the template's own parameters, each a small non-negative integer (below 1024), at most six of them; an argument out of that range
// gives KEY_NONE, which no row has
constexpr uint64_t KEY_NONE = ~0ull;
constexpr uint64_t kernel_key() { return 0; }
template <typename... I> constexpr uint64_t kernel_key(int f, I... rest) {
  static_assert(sizeof...(I) < 6, "six fields of ten bits");
  const uint64_t r = kernel_key(rest...);
  return ((unsigned)f >> 10) || r == KEY_NONE ? KEY_NONE : (r << 10 | (unsigned)f);
}

struct KernelRow {
  uint64_t key;        // kernel_key(the template's own parameters)
  const void* fn;      // the instantiation
  uint32_t lds;        // dynamic LDS bytes
  uint32_t threads;    // workgroup size
};
struct KernelTable {
  const KernelRow* rows;
  int n;
  template <int N> constexpr KernelTable(const KernelRow (&r)[N]) : rows(r), n(N) {}
};

inline const KernelRow* find(const KernelTable& t, uint64_t key) {
  for (int i = 0; i < t.n; ++i)
    if (t.rows[i].key == key) return &t.rows[i];
  return nullptr;
}
inline hipError_t set_lds_all(const KernelTable& t) {
  for (int i = 0; i < t.n; ++i) {
    const hipError_t e = hipFuncSetAttribute(t.rows[i].fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)t.rows[i].lds);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}
// args: the kernel's parameters, exactly as the __global__ function declares them, in type, order and count.  They travel as void*: unlike
// hipLaunchKernelGGL nothing checks them against the kernel, and a wrong or missing one compiles and runs on garbage.  Every table's rows share one
// parameter list (its file's *Args struct; gemm2 and the ablation build's gemm4 take a second `int flags`), stated at each call.
template <typename... A> hipError_t launch(const KernelRow& r, dim3 grid, hipStream_t s, const A&... args) {
  void* p[] = {const_cast<void*>(static_cast<const void*>(&args))...};
  (void)hipLaunchKernel(r.fn, grid, dim3(r.threads), p, r.lds, s);
  return hipGetLastError();
}

// the seven tables, in the order of ns2vc_debug_kernel_table's `family`
const KernelTable& gemm2_kernel_table();
const KernelTable& gemm4_kernel_table();
const KernelTable& conv3ts_kernel_table();
const KernelTable& attn_kernel_table();
const KernelTable& ffn_kernel_table();
const KernelTable& geglu_kernel_table();
const KernelTable& rowchain_kernel_table();
// (not a family of ns2vc_debug_kernel_table: ns2vc_debug_attnres_table)
const KernelTable& attnres_kernel_table();
const KernelTable& attnres_lens_kernel_table();      // (ns2vc_debug_attnres_lens_table)

}  // namespace ns2vc
