// Clipped Adam over a device table of tensors (include/temp_amd.h: temp_grad_norm_clip, temp_adam_clip_step): the trainer's
// clip_grad_norm_ + Adam(weight_decay) as a norm pass, a one-block finish and an update pass.
//
// The work list is the tensors' CHUNKS: TEMP_ADAM_CHUNK consecutive elements of one tensor (the last chunk of a tensor is short),
// numbered through the table in row order; row t owns chunks [first_chunk[t], first_chunk[t + 1]).  A workgroup takes chunk
// blockIdx.x, blockIdx.x + gridDim.x, ... (the grid is capped, guide section 6 guideline 11) and finds the chunk's row by a binary
// search over the first-chunk column -- block-uniform, so the row's pointers and scalars are scalar loads.  Inside a chunk lane l
// owns elements [4 l + 1024 i, 4 l + 1024 i + 4): one float4 access each when the row's pointers are 16-byte aligned (a chunk
// starts a multiple of 16 KB behind them), four scalar accesses otherwise (a parameter that is a view at a 4-byte offset).  The
// assignment of elements to lanes is the same on both routes, so neither result depends on the alignment.
//
// Norm pass: a lane squares and adds its elements in double (the square of an fp32 value is exact in double), in index order;
// the 64 lanes of a wave are added by a butterfly, the four waves in wave order, and the chunk's sum is stored to partial[chunk]
// -- no atomics.  k_adam_norm_finish (one workgroup) adds the partials -- thread t those with index t mod 256, ascending, then a
// tree over the threads -- and stores norm and the clip coefficient as two floats.  Every order is a function of the table alone:
// the same gradients give the same bits, whatever the grid.
//
// Update pass: reads the coefficient from device memory (NULL: 1) and applies step 3 of the contract in place, in fp32, with the
// row's scalars.  Nothing here special-cases a non-finite value: an infinite norm gives coef = 0, a NaN norm coef = NaN.
#include "common.hpp"

namespace temp {
namespace {

constexpr int ADAM_THREADS = 256;
constexpr int ADAM_MAX_GRID = 2048;
static_assert(TEMP_ADAM_CHUNK % (ADAM_THREADS * 4) == 0, "a chunk is whole float4 rounds of the workgroup");

// row of the table that owns `chunk`: the last one whose first chunk is <= chunk (rows without elements own no chunk and share
// their first chunk with the row behind them, which this rule skips to)
__device__ __forceinline__ int adam_row_of(const TempAdamTensor* __restrict__ tab, int n_tensors, int chunk) {
  int lo = 0, hi = n_tensors - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tab[mid].first_chunk <= chunk) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__device__ __forceinline__ bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// elements [i, i + 4) of a chunk of `len` elements; slots at or behind len read as 0 and are not stored
template <bool VEC>
__device__ __forceinline__ float4 adam_load(const float* __restrict__ p, long long i, long long len) {
  if (VEC && i + 4 <= len) return ld4(p + i);
  float4 r = zero4();
  if (i < len) r.x = p[i];
  if (i + 1 < len) r.y = p[i + 1];
  if (i + 2 < len) r.z = p[i + 2];
  if (i + 3 < len) r.w = p[i + 3];
  return r;
}
template <bool VEC>
__device__ __forceinline__ void adam_store(float* __restrict__ p, long long i, long long len, float4 x) {
  if (VEC && i + 4 <= len) { st4(p + i, x); return; }
  if (i < len) p[i] = x.x;
  if (i + 1 < len) p[i + 1] = x.y;
  if (i + 2 < len) p[i + 2] = x.z;
  if (i + 3 < len) p[i + 3] = x.w;
}

// sum of squares of a lane's elements of one chunk, in index order on every route
template <bool VEC>
__device__ __forceinline__ double norm_chunk(const float* __restrict__ g, int len) {
  constexpr int ROUNDS = TEMP_ADAM_CHUNK / (ADAM_THREADS * 4);
  double acc = 0.0;
  if (len == TEMP_ADAM_CHUNK) {                                   // a whole chunk: every load in flight before the first add
    float x[ROUNDS][4];
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
      const float* q = g + (r * ADAM_THREADS + threadIdx.x) * 4;
      if (VEC) {
        const float4 t = ld4(q);
        x[r][0] = t.x; x[r][1] = t.y; x[r][2] = t.z; x[r][3] = t.w;
      } else {
        x[r][0] = q[0]; x[r][1] = q[1]; x[r][2] = q[2]; x[r][3] = q[3];
      }
    }
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r)
#pragma unroll
      for (int k = 0; k < 4; ++k) acc = fma((double)x[r][k], (double)x[r][k], acc);
    return acc;
  }
#pragma unroll 1
  for (int r = 0; r < ROUNDS; ++r) {                              // a tensor's last chunk: element by element (kept small: few registers
    const int i = (r * ADAM_THREADS + threadIdx.x) * 4;           // here keep the whole-chunk route at eight waves per SIMD)
#pragma unroll 1
    for (int k = i; k < min(i + 4, len); ++k) acc = fma((double)g[k], (double)g[k], acc);
  }
  return acc;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m);
  return v;
}

__global__ void __launch_bounds__(ADAM_THREADS) k_adam_grad_norm(int n_tensors, int n_chunks, const TempAdamTensor* __restrict__ tab,
                                                                 double* __restrict__ partial) {
  __shared__ double wsum[ADAM_THREADS / TEMP_WAVE];
  for (int chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
    const TempAdamTensor& row = tab[adam_row_of(tab, n_tensors, chunk)];
    const long long off = (long long)(chunk - row.first_chunk) * TEMP_ADAM_CHUNK;
    long long len = row.n - off;                                   // <= 0 only for a table whose chunk count overstates its rows
    len = len > TEMP_ADAM_CHUNK ? TEMP_ADAM_CHUNK : len;
    const float* g = row.g + off;
    double acc = 0.0;
    if (len > 0) acc = aligned16(row.g) ? norm_chunk<true>(g, (int)len) : norm_chunk<false>(g, (int)len);
    acc = wave_sum(acc);
    if ((threadIdx.x & (TEMP_WAVE - 1)) == 0) wsum[threadIdx.x / TEMP_WAVE] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[chunk] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
    __syncthreads();                                               // wsum is written again by the next chunk
  }
}

__global__ void __launch_bounds__(ADAM_THREADS) k_adam_norm_finish(int n_chunks, const double* __restrict__ partial, double max_norm,
                                                                   float* __restrict__ norm_coef) {
  __shared__ double s[ADAM_THREADS];
  double acc = 0.0;
  for (int i = threadIdx.x; i < n_chunks; i += ADAM_THREADS) acc += partial[i];
  s[threadIdx.x] = acc;
  __syncthreads();
  for (int w = ADAM_THREADS / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) s[threadIdx.x] += s[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double norm = sqrt(s[0]);
    const double r = max_norm / (norm + 1e-6);
    const double coef = (r < 1.0 || r != r) ? r : 1.0;             // min(r, 1) that lets a NaN through, as torch's clamp does
    norm_coef[0] = (float)norm;
    norm_coef[1] = (float)coef;
  }
}

template <bool VEC>
__device__ __forceinline__ void adam_chunk(const TempAdamTensor& row, long long off, long long len, float coef) {
  float* __restrict__ p = row.p + off;
  const float* __restrict__ g = row.g + off;
  float* __restrict__ m = row.m + off;
  float* __restrict__ v = row.v + off;
  const float step_size = row.step_size, inv_bc2 = row.inv_bias2_sqrt, b2 = row.beta2, eps = row.eps, wd = row.weight_decay;
  const float omb1 = row.one_minus_beta1, omb2 = row.one_minus_beta2;
  constexpr int ROUNDS = TEMP_ADAM_CHUNK / (ADAM_THREADS * 4);
  float4 xp[ROUNDS], xg[ROUNDS], xm[ROUNDS], xv[ROUNDS];
#pragma unroll
  for (int r = 0; r < ROUNDS; ++r) {                               // every load of the chunk in flight before the first use
    const long long i = ((long long)r * ADAM_THREADS + threadIdx.x) * 4;
    xp[r] = adam_load<VEC>(p, i, len);
    xg[r] = adam_load<VEC>(g, i, len);
    xm[r] = adam_load<VEC>(m, i, len);
    xv[r] = adam_load<VEC>(v, i, len);
  }
#pragma unroll
  for (int r = 0; r < ROUNDS; ++r) {
    const long long i = ((long long)r * ADAM_THREADS + threadIdx.x) * 4;
    if (i >= len) continue;
    float ep[4] = {xp[r].x, xp[r].y, xp[r].z, xp[r].w};
    const float eg[4] = {xg[r].x, xg[r].y, xg[r].z, xg[r].w};
    float em[4] = {xm[r].x, xm[r].y, xm[r].z, xm[r].w};
    float ev[4] = {xv[r].x, xv[r].y, xv[r].z, xv[r].w};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float gq = fmaf(wd, ep[q], coef * eg[q]);
      em[q] = fmaf(omb1, gq - em[q], em[q]);
      ev[q] = fmaf(omb2, gq * gq, b2 * ev[q]);
      const float denom = fmaf(sqrtf(ev[q]), inv_bc2, eps);
      ep[q] = fmaf(-step_size, em[q] / denom, ep[q]);
    }
    adam_store<VEC>(p, i, len, make_float4(ep[0], ep[1], ep[2], ep[3]));
    adam_store<VEC>(m, i, len, make_float4(em[0], em[1], em[2], em[3]));
    adam_store<VEC>(v, i, len, make_float4(ev[0], ev[1], ev[2], ev[3]));
  }
}

__global__ void __launch_bounds__(ADAM_THREADS) k_adam_clip_step(int n_tensors, int n_chunks, const TempAdamTensor* __restrict__ tab,
                                                                 const float* __restrict__ norm_coef) {
  const float coef = norm_coef ? norm_coef[1] : 1.0f;
  for (int chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
    const TempAdamTensor& row = tab[adam_row_of(tab, n_tensors, chunk)];
    const long long off = (long long)(chunk - row.first_chunk) * TEMP_ADAM_CHUNK;
    long long len = row.n - off;
    len = len > TEMP_ADAM_CHUNK ? TEMP_ADAM_CHUNK : len;
    if (len <= 0) continue;
    if (aligned16(row.p) && aligned16(row.g) && aligned16(row.m) && aligned16(row.v)) adam_chunk<true>(row, off, len, coef);
    else adam_chunk<false>(row, off, len, coef);
  }
}

inline int adam_grid(int n_chunks) { return n_chunks < ADAM_MAX_GRID ? n_chunks : ADAM_MAX_GRID; }

}  // namespace
}  // namespace temp

using namespace temp;

extern "C" {

size_t temp_grad_norm_workspace(int n_chunks) {
  Carver c(nullptr);
  c.take((size_t)(n_chunks > 0 ? n_chunks : 0) * sizeof(double));
  return c.total();
}

int temp_grad_norm_clip(int n_tensors, int n_chunks, const TempAdamTensor* table, double max_norm, void* ws, size_t ws_bytes,
                        float* norm_coef, void* stream) {
  if (n_tensors < 0 || n_chunks < 0 || !norm_coef || (n_chunks > 0 && (n_tensors == 0 || !table))) return TEMP_E_BADARG;
  if (reinterpret_cast<uintptr_t>(ws) % sizeof(double)) return TEMP_E_BADARG;
  if (n_chunks > 0 && (!ws || ws_bytes < temp_grad_norm_workspace(n_chunks))) return TEMP_E_WORKSPACE;
  Carver c(ws);
  double* partial = reinterpret_cast<double*>(c.take((size_t)n_chunks * sizeof(double)));
  hipStream_t st = (hipStream_t)stream;
  if (n_chunks > 0) TEMP_LAUNCH(K_ADAM_GRAD_NORM, k_adam_grad_norm, dim3(adam_grid(n_chunks)), dim3(ADAM_THREADS), 0, st, n_tensors, n_chunks, table, partial);
  TEMP_LAUNCH(K_ADAM_NORM_FINISH, k_adam_norm_finish, dim3(1), dim3(ADAM_THREADS), 0, st, n_chunks, partial, max_norm, norm_coef);
  return launch_status();
}

int temp_adam_clip_step(int n_tensors, int n_chunks, const TempAdamTensor* table, const float* norm_coef, void* stream) {
  if (n_tensors < 0 || n_chunks < 0 || (n_chunks > 0 && (n_tensors == 0 || !table))) return TEMP_E_BADARG;
  if (n_chunks == 0) return TEMP_OK;
  TEMP_LAUNCH(K_ADAM_CLIP_STEP, k_adam_clip_step, dim3(adam_grid(n_chunks)), dim3(ADAM_THREADS), 0, (hipStream_t)stream, n_tensors, n_chunks, table,
              norm_coef);
  return launch_status();
}

}  // extern "C"
