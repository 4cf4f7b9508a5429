// The library's runtime state and the entry points that belong to no kernel family: the kernel-selection switches
// (include/temp_amd.h: temp_set_option) with their environment defaults, the optional per-kernel trace behind TEMP_LAUNCH, the
// ABI version and error strings, the diagnostic counter of f16-split launches, and the copy probe.
#include "common.hpp"
#include <atomic>
#include <cstdlib>

namespace temp {

__global__ void __launch_bounds__(256) k_copy(size_t n16, const float4* __restrict__ src, float4* __restrict__ dst) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (size_t)gridDim.x * blockDim.x) dst[i] = src[i];
}

// ---- trace state -------------------------------------------------------------------------------
struct TraceState { hipEvent_t* ev; int* ids; int cap; int n; };
static TraceState* g_trace = nullptr;

int trace_open(int kernel_id, hipStream_t st) {
  TraceState* t = g_trace;
  if (!t) return -1;
  const int slot = __atomic_fetch_add(&t->n, 1, __ATOMIC_RELAXED);
  if (slot >= t->cap) return -1;
  t->ids[slot] = kernel_id;
  (void)hipEventRecord(t->ev[2 * slot], st);
  return slot;
}
void trace_close(int slot, hipStream_t st) {
  TraceState* t = g_trace;
  if (!t || slot < 0) return;
  (void)hipEventRecord(t->ev[2 * slot + 1], st);
}

}  // namespace temp

using namespace temp;

extern "C" {

int temp_trace_begin(int capacity) {
  if (capacity <= 0 || g_trace) return TEMP_E_BADARG;
  TraceState* t = new TraceState();
  t->cap = capacity;
  t->n = 0;
  t->ids = new int[capacity];
  t->ev = new hipEvent_t[2 * (size_t)capacity];
  for (int i = 0; i < 2 * capacity; ++i)
    if (hipEventCreate(&t->ev[i]) != hipSuccess) return TEMP_E_LAUNCH;
  g_trace = t;
  return TEMP_OK;
}

int temp_trace_end(int* kernel_ids, float* ms, int capacity, int* n_out) {
  TraceState* t = g_trace;
  if (!t || !n_out) return TEMP_E_BADARG;
  g_trace = nullptr;
  if (hipDeviceSynchronize() != hipSuccess) return TEMP_E_LAUNCH;
  int n = t->n < t->cap ? t->n : t->cap;
  if (n > capacity) n = capacity;
  for (int i = 0; i < n; ++i) {
    float v = 0.f;
    (void)hipEventElapsedTime(&v, t->ev[2 * i], t->ev[2 * i + 1]);
    if (kernel_ids) kernel_ids[i] = t->ids[i];
    if (ms) ms[i] = v;
  }
  *n_out = n;
  for (int i = 0; i < 2 * t->cap; ++i) (void)hipEventDestroy(t->ev[i]);
  delete[] t->ev;
  delete[] t->ids;
  delete t;
  return TEMP_OK;
}

}  // extern "C"

namespace temp {
// ---- kernel-selection switches (include/temp_amd.h).  Defaults, then the environment, once at load time.
static std::atomic<int> g_options[TEMP_OPT_COUNT];
static const bool g_options_init = [] {
  g_options[TEMP_OPT_MFMA_BF16X3] = 1; g_options[TEMP_OPT_TN_SPLIT] = 1; g_options[TEMP_OPT_RGCN_SCALAR] = 1;
  g_options[TEMP_OPT_GEMM_STREAM] = 0; g_options[TEMP_OPT_GRU_STREAM] = 0; g_options[TEMP_OPT_RGCN_TILE] = 1; g_options[TEMP_OPT_DEBUG] = 0; g_options[TEMP_OPT_OVERLAP] = 1; g_options[TEMP_OPT_GEMM_RESIDENT] = 1;
  g_options[TEMP_OPT_MFMA_F16X2] = 1;
  g_options[TEMP_OPT_RGCN_PAIR] = 1;
  const char* e;
  if ((e = getenv("TEMP_MFMA")) && e[0] == 'f' && e[1] == '3') g_options[TEMP_OPT_MFMA_BF16X3] = 0;      // f32
  if ((e = getenv("TEMP_MFMA")) && e[0] == 'b') g_options[TEMP_OPT_MFMA_F16X2] = 0;                       // bf16x3
  if ((e = getenv("TEMP_TN_SPLIT")) && e[0] == '0') g_options[TEMP_OPT_TN_SPLIT] = 0;
  if ((e = getenv("TEMP_RGCN_SCALAR")) && e[0] == '0') g_options[TEMP_OPT_RGCN_SCALAR] = 0;
  if ((e = getenv("TEMP_GEMM_STREAM")) && e[0] == '1') g_options[TEMP_OPT_GEMM_STREAM] = 1;
  if ((e = getenv("TEMP_GRU_STREAM")) && e[0] == '1') g_options[TEMP_OPT_GRU_STREAM] = 1;
  if ((e = getenv("TEMP_RGCN_TILE")) && e[0] >= '0' && e[0] <= '9') g_options[TEMP_OPT_RGCN_TILE] = atoi(e);
  if ((e = getenv("TEMP_OVERLAP")) && e[0] == '0') g_options[TEMP_OPT_OVERLAP] = 0;
  if ((e = getenv("TEMP_GEMM_RESIDENT")) && e[0] == '0') g_options[TEMP_OPT_GEMM_RESIDENT] = 0;
  if ((e = getenv("TEMP_DEBUG"))) g_options[TEMP_OPT_DEBUG] = atoi(e);
  if ((e = getenv("TEMP_RGCN_PAIR")) && e[0] >= '0' && e[0] <= '9') g_options[TEMP_OPT_RGCN_PAIR] = atoi(e);
  return true;
}();
int option(int key) { return (key >= 0 && key < TEMP_OPT_COUNT) ? g_options[key].load(std::memory_order_relaxed) : -1; }
static std::atomic<long long> g_hx_launches{0};
void hx_count() { g_hx_launches.fetch_add(1, std::memory_order_relaxed); }
long long hx_launches() { return g_hx_launches.load(std::memory_order_relaxed); }
static std::atomic<long long> g_gemm_routes[TEMP_ROUTE_COUNT][8];       // (static storage: zero)
void gemm_route_count(int route, int width) {
  if (route >= 0 && route < TEMP_ROUTE_COUNT && width >= 0 && width < 8) g_gemm_routes[route][width].fetch_add(1, std::memory_order_relaxed);
}
long long gemm_route_launches(int route, int width) {
  if (route < 0 || route >= TEMP_ROUTE_COUNT || width < 0 || width >= 8) return -1;
  return g_gemm_routes[route][width].load(std::memory_order_relaxed);
}
static std::atomic<long long> g_rgcn_routes[TEMP_RGCN_ROUTE_COUNT][5];  // (static storage: zero)
void rgcn_route_count(int route, int s) {
  if (route >= 0 && route < TEMP_RGCN_ROUTE_COUNT && s >= 0 && s < 5) g_rgcn_routes[route][s].fetch_add(1, std::memory_order_relaxed);
}
long long rgcn_route_launches(int route, int s) {
  if (route < 0 || route >= TEMP_RGCN_ROUTE_COUNT || s < 0 || s >= 5) return -1;
  return g_rgcn_routes[route][s].load(std::memory_order_relaxed);
}
static std::atomic<long long> g_gru_routes[TEMP_GRU_ROUTE_COUNT];       // (static storage: zero)
void gru_route_count(int route) {
  if (route >= 0 && route < TEMP_GRU_ROUTE_COUNT) g_gru_routes[route].fetch_add(1, std::memory_order_relaxed);
}
long long gru_route_launches(int route) {
  if (route < 0 || route >= TEMP_GRU_ROUTE_COUNT) return -1;
  return g_gru_routes[route].load(std::memory_order_relaxed);
}
}  // namespace temp

extern "C" {

const char* temp_trace_kernel_name(int id) {
  static const char* names[] = {"k_rgcn_agg<fwd>", "k_rgcn_agg<dx>", "k_rgcn_dw", "k_fixup", "k_gemm_panel<loop_fwd>",
                                "k_gemm_panel<loop_dx>", "k_gemm_tn", "k_reduce_slices", "k_colsum_part", "k_relu_bwd", "k_gru_fwd",
                                "k_gru_bwd_gates", "k_gemm_panel<gru_dx>", "k_gemm_panel<gru_dprev>", "k_gather_rows",
                                "k_scatter_add_rows", "k_decay_grad", "k_copy", "k_gemm_panel<isolated>", "k_gemm_panel<gru_gi>",
                                "k_gemm_panel<linear>", "k_gather_ce", "k_sa_attn_fwd", "k_sa_attn_bwd", "k_gru_chain_fwd", "k_gru_chain_bwd",
                                "k_gru_chain_pack", "k_bx_pack", "k_gemm_tn_bx8", "k_gemm_tn_bx", "k_gru_wgrad", "k_segment_sum_rows", "k_absmax_keys",
                                "k_gated_query", "k_gather_ce_mix", "k_pair_msg", "k_pair_gather<fwd>", "k_pair_fix_epi", "k_pair_gather<bwd>",
                                "k_pair_tail", "k_diachronic_fwd", "k_diachronic_bwd", "k_filtered_topk", "k_adam_grad_norm", "k_adam_norm_finish",
                                "k_adam_clip_step", "k_filtered_topk_mix", "k_hyperplane_fwd", "k_hyperplane_bwd", "k_hyperplane_bwd_finish",
                                "k_pair_rows_fwd", "k_pair_rows_bwd", "k_frozen_mix_ce", "k_filtered_ce_fwd", "k_filtered_ce_bwd",
                                "k_filtered_rank_stream", "k_filtered_rank_stream_mix", "k_dot_ce_fwd", "k_dot_ce_bwd_q",
                                "k_dot_ce_bwd_table", "k_dot_mix_ce_fwd", "k_dot_mix_ce_bwd_q", "k_dot_mix_ce_bwd_table",
                                "k_lin_chain_fwd", "k_lin_chain_bwd", "k_lin_chain_pack", "k_lin_rows_fwd", "k_lin_rows_bwd",
                                "k_lin_rows2_fwd", "k_lin_rows2_bwd"};
  static_assert(sizeof(names) / sizeof(names[0]) == K_COUNT, "one name per KernelId");
  return (id >= 0 && id < K_COUNT) ? names[id] : "?";
}

int temp_abi_version(void) { return TEMP_ABI_VERSION; }

int temp_set_option(int key, int value) {
  if (key < 0 || key >= TEMP_OPT_COUNT) return -1;
  return temp::g_options[key].exchange(value, std::memory_order_relaxed);
}
int temp_get_option(int key) { return temp::option(key); }
long long temp_f16_launches(void) { return temp::hx_launches(); }
long long temp_gemm_route_launches(int route, int width) { return temp::gemm_route_launches(route, width); }
long long temp_rgcn_route_launches(int route, int s) { return temp::rgcn_route_launches(route, s); }
long long temp_gru_route_launches(int route) { return temp::gru_route_launches(route); }

const char* temp_error_string(int code) {
  switch (code) {
    case TEMP_OK: return "ok";
    case TEMP_E_BADARG: return "bad argument (NULL, negative or inconsistent)";
    case TEMP_E_UNSUPPORTED: return "shape not supported by the gfx950 kernels";
    case TEMP_E_WORKSPACE: return "workspace missing or too small";
    case TEMP_E_LAUNCH: return "HIP launch failure";
    default: return "unknown error";
  }
}

int temp_copy_probe(const void* src, void* dst, size_t bytes, void* stream) {
  if (!src || !dst || bytes % 16) return TEMP_E_BADARG;
  if (bytes == 0) return TEMP_OK;
  TEMP_LAUNCH(K_COPY, k_copy, dim3(2048), dim3(256), 0, (hipStream_t)stream, bytes / 16, (const float4*)src, (float4*)dst);
  return launch_status();
}

}  // extern "C"
