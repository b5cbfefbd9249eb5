// Dev tool: per-wave timeline of one launch of the split GEMM's 256 x 256 form (gemm_split_bf16_v3_kernel compiled with its DF_STRACE hooks on):
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -Wno-unused-value -I include -o tools/dev/split_gemm_trace tools/dev/split_gemm_trace.hip densefusion_amd/csrc/common.hip
//   tools/dev/split_gemm_trace M N K colsum_only workgroups [tag]
// colsum_only 1: per-group bias (1 024-row groups, 1 000 real rows), fused column sums, no output buffer; workgroups: -1 one per compute unit (the
// product's launch), 0 one per tile position (no walk), N a limit.  Prints one JSON line of per-phase medians in microseconds.
// Stamps per wave and tile (100 MHz wall clock, written by lane 0 with ordinary vector stores): 0 kernel entry (filed under the workgroup's first
// tile), 1 the tile's first loads issued (in a walk: ahead of the previous tile's epilogue), 2 first barrier passed (stage 0 cut and written), 3 main
// loop left, 4 first 64-row block through LDS and its stores issued, 5 last store issued, 6 wave end (under the workgroup's last tile).
#include <hip/hip_runtime.h>
__device__ unsigned long long *df_strace_buf = nullptr;
#define DF_STRACE_ENTRY() const unsigned long long strace_t0 = wall_clock64()
#define DF_STRACE(i, s)                                                                                                        \
  do {                                                                                                                         \
    if ((threadIdx.x & 63) == 0 && df_strace_buf) {                                                                            \
      unsigned long long *r = df_strace_buf + (((size_t)(s) * 8 + (blockIdx.x & 7)) * 8 + (threadIdx.x >> 6)) * 8;              \
      r[i] = (i) == 0 ? strace_t0 : wall_clock64();                                                                            \
      if ((i) == 1)                                                                                                            \
        r[7] = (unsigned long long)(__builtin_amdgcn_s_getreg((3 << 11) | 20) & 7) << 32 | __builtin_amdgcn_s_getreg((31 << 11) | 4); \
    }                                                                                                                          \
  } while (0)
#include "../../densefusion_amd/csrc/split_gemm.hip"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>
using namespace df;

__global__ void fill_kernel(float *x, size_t n, unsigned seed, float scale) {          // post-ReLU-like: non-negative, a third of them zero
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    unsigned h = (unsigned)i * 2654435761u ^ seed;
    h ^= h >> 15; h *= 2246822519u; h ^= h >> 13;
    x[i] = (h % 3 == 0) ? 0.f : scale * (float)(h >> 8) * (1.f / 16777216.f);
  }
}

static double median(std::vector<double> v) {
  if (v.empty()) return -1;
  std::sort(v.begin(), v.end());
  return v[v.size() / 2];
}

int main(int argc, char **argv) {
  const long M = argc > 1 ? atol(argv[1]) : 139000;
  const int N = argc > 2 ? atoi(argv[2]) : 1024, K = argc > 3 ? atoi(argv[3]) : 512, cs_only = argc > 4 ? atoi(argv[4]) : 0;
  const int workgroups = argc > 5 ? atoi(argv[5]) : -1;
  const char *tag = argc > 6 ? argv[6] : "";
  float *x, *w, *b, *out = nullptr, *cs = nullptr;
  __bf16 *planes;
  const long groups = cs_only ? M / 1024 : 1;
  if (cs_only && M % 1024) { fprintf(stderr, "colsum_only needs M %% 1024 == 0\n"); return 2; }
  hipMalloc(&x, (size_t)M * K * 4); hipMalloc(&w, (size_t)N * K * 4); hipMalloc(&planes, (size_t)N * K * 3 * 2); hipMalloc(&b, (size_t)groups * N * 4);
  if (cs_only) hipMalloc(&cs, (size_t)colsum_partial_rows(M) * N * 4); else hipMalloc(&out, (size_t)M * N * 4);
  hipLaunchKernelGGL(fill_kernel, dim3(4096), dim3(256), 0, 0, x, (size_t)M * K, 1u, 1.f);
  hipLaunchKernelGGL(fill_kernel, dim3(1024), dim3(256), 0, 0, w, (size_t)N * K, 2u, 0.05f);
  hipLaunchKernelGGL(fill_kernel, dim3(64), dim3(256), 0, 0, b, (size_t)groups * N, 3u, 1.f);
  cut_weight_planes(w, planes, (long)N * K, (long)N * K, 0);
  ConvParams p;
  p.in = x; p.wgt = w; p.wpl = planes; p.wpl_stride = (long)N * K; p.bias = b; p.out = out; p.colsum = cs;
  p.B = (int)M; p.Cin = K; p.in_ld = K; p.Cout = N; p.out_ld = N; p.act = ACT_RELU;
  if (cs_only) { p.rows_per_group = 1024; p.rows_valid = 1000; p.bias_group_ld = N; }
  int cus = 256;
  hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0);
  SplitPlan pl;
  if (plan_split(p, cus, 3, false, workgroups, pl) != 1 || pl.form != FORM_256x256) { fprintf(stderr, "the launch does not take the 256 x 256 form\n"); return 2; }
  if (raise_lds_limit(reinterpret_cast<const void *>(gemm_split_bf16_v3_kernel), pl.lds) != DF_OK) return 3;
  auto launch = [&] { hipLaunchKernelGGL(gemm_split_bf16_v3_kernel, pl.grid, dim3(pl.threads), pl.lds, 0, pl.a); };
  hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
  for (int i = 0; i < 3; ++i) launch();
  hipEventRecord(e0);
  for (int i = 0; i < 10; ++i) launch();
  hipEventRecord(e1); hipEventSynchronize(e1);
  float ms; hipEventElapsedTime(&ms, e0, e1);
  if (hipGetLastError() != hipSuccess) { fprintf(stderr, "launch failed\n"); return 4; }
  const size_t recs = (size_t)pl.a.tiles_total * 8;          // (tile position, wave)
  unsigned long long *buf;
  hipMalloc(&buf, recs * 64); hipMemset(buf, 0, recs * 64);
  hipMemcpyToSymbol(HIP_SYMBOL(df_strace_buf), &buf, sizeof(buf));
  launch();
  if (hipDeviceSynchronize() != hipSuccess) { fprintf(stderr, "traced launch failed\n"); return 4; }
  std::vector<unsigned long long> h(recs * 8);
  hipMemcpy(h.data(), buf, recs * 64, hipMemcpyDeviceToHost);

  // walk every workgroup's tiles in its order, wave by wave
  const int grid = (int)pl.grid.x, step = grid / 8, seqs = pl.a.tiles_total / 8;
  std::vector<double> entry_to_loads, first_to_barrier, handover, main_loop, block0, block1, tile_period, gaps;
  std::map<unsigned long long, std::vector<std::pair<unsigned long long, unsigned long long>>> per_cu;          // CU -> (entry, end) of its workgroups (wave 0)
  long tiles = 0;
  unsigned long long t_first = ~0ull, t_last = 0;
  for (int wgi = 0; wgi < grid; ++wgi)
    for (int wave = 0; wave < 8; ++wave) {
      const unsigned long long *prev = nullptr, *first = nullptr;
      for (int s = wgi / 8; s < seqs; s += step) {
        const unsigned long long *r = &h[(((size_t)s * 8 + (wgi & 7)) * 8 + wave) * 8];
        if (!r[2]) continue;          // a padding position
        if (wave == 0) ++tiles;
        if (!first) { first = r; entry_to_loads.push_back((double)(r[1] - r[0])); first_to_barrier.push_back((double)(r[2] - r[0])); }
        else { handover.push_back((double)(r[2] - prev[5])); tile_period.push_back((double)(r[2] - prev[2])); }
        main_loop.push_back((double)(r[3] - r[2])); block0.push_back((double)(r[4] - r[3])); block1.push_back((double)(r[5] - r[4]));
        t_first = std::min(t_first, r[first == r ? 0 : 2]); t_last = std::max(t_last, r[5]);
        prev = r;
      }
      // (HW_ID bits 8 .. 15: CU, shader array, shader engine; the XCC id above them)
      if (first && wave == 0) per_cu[(first[7] >> 32) << 8 | ((first[7] >> 8) & 0xff)].push_back({first[0], prev[6]});
    }
  for (auto &kv : per_cu) {          // one workgroup's end to the next one's entry on the same CU
    std::sort(kv.second.begin(), kv.second.end());
    for (size_t i = 1; i < kv.second.size(); ++i) gaps.push_back((double)kv.second[i].first - (double)kv.second[i - 1].second);
  }
  const double us = 0.01;          // 100 MHz
  printf("{\"tag\": \"%s\", \"M\": %ld, \"N\": %d, \"K\": %d, \"colsum_only\": %d, \"workgroups\": %d, \"tiles\": %ld, \"cus_seen\": %zu, \"launch_us\": %.1f, "
         "\"traced_span_us\": %.1f, \"median_us\": {\"entry_to_first_loads\": %.2f, \"entry_to_first_barrier\": %.2f, \"last_store_to_next_first_barrier\": %.2f, "
         "\"main_loop\": %.2f, \"next_fetches_and_block0_epilogue\": %.2f, \"block1_epilogue\": %.2f, \"first_barrier_to_next_first_barrier\": %.2f, "
         "\"workgroup_end_to_next_entry_same_cu\": %.2f}}\n",
         tag, M, N, K, cs_only, grid, tiles, per_cu.size(), ms * 100, (double)(t_last - t_first) * us, median(entry_to_loads) * us, median(first_to_barrier) * us,
         median(handover) * us, median(main_loop) * us, median(block0) * us, median(block1) * us, median(tile_period) * us, median(gaps) * us);
  return 0;
}
