// Persistent window chain of the LINEAR recurrence on gfx950 (include/temp_amd.h: TempLinChain).
//
//   h_p = act(x_p + (exp(-lambda dt) h_{p-1}) . W)        RRGCNLayer / BiRRGCNLayer (models/RRGCN.py:120-167, models/BiRRGCN.py:102-185)
//
// The structure is that of gru_chain.hip and the tables are its tables, unchanged: a workgroup owns a PANEL of 32 entity tracks, keeps
// their states in LDS and walks every step of the panel inside one launch.  Per step the product is 32 x d x d (one third of the GRU's,
// no gates) on v_mfma_f32_32x32x2_f32, W streamed from L2 in fragment order (k_lin_chain_pack).  All arithmetic is fp32: there is no
// tanh, so the state has no bound a constant-scale f16 split could use.
//
// 256 threads (four waves), no role split: a step is three phases of the whole workgroup with two barriers,
//   1  rows     every thread owns fixed (track, 4 columns) items: the decayed state (forward) / d_pre (backward) of the step is formed,
//               written to global memory row-contiguously and left in LDS as the B operand (k padded with zeros);
//   2  product  wave w owns column tiles w, w + 4 (two independent accumulators); raw products go back to LDS;
//   3  rows     (forward only) x + product, activation, h to global memory and to LDS as the next step's state -- by the thread
//               that reads it in phase 1 of the next step, so no barrier separates the two.
// The backward needs no third phase: d_prev stays raw in LDS and the successor's decay is applied where phase 1 of the step before adds
// it to the upstream gradient.  No atomics; every sum has one order per launch shape, so results are bit-repeatable.  Several
// workgroups share a CU (60 KB of LDS at d = 200), which is what hides the L2 latency of the weight stream in this plain version.
//
// k_lin_rows_fwd<NS> / _bwd<NS> are ONE such step on gathered rows, without the tables, with NS history sources in front of one
// activation.  NS = 1 (temp_lin_rows_*): the (window, entity) pair rows of the batched all-entity pass.  NS = 2 (temp_lin_rows2_*): both
// directions' recurrent terms, BiRRGCNLayer's centre position and its union pair rows.
#include <atomic>
#include "common.hpp"

namespace temp {

#define LC_TRACKS TEMP_CHAIN_TRACKS
#define LC_HAS_PREV TEMP_CHAIN_HAS_PREV
#define LC_ROW_MASK (TEMP_CHAIN_HAS_PREV - 1)
#define LC_MAX_STEPS 64
#define LC_THREADS 256
#define LC_LDS_LIMIT (160 * 1024)

struct LinGeom {
  int NT, NQ;        // tiles of 32 columns, k-groups of 8 (both over d: the matrix is square)
  int ldo, ldk;      // LDS strides (floats): product / state rows, B-operand rows; (stride / 4) odd: conflict-free b128 accesses across rows
};
__host__ __device__ inline LinGeom lin_geom(int D) {
  LinGeom g;
  g.NT = (D + 31) >> 5; g.NQ = (D + 7) >> 3;
  g.ldo = g.NT * 32 + 4; g.ldk = g.NQ * 8 + 4;
  return g;
}
inline size_t lin_lds_fwd(int D, int ms) { LinGeom g = lin_geom(D); return ((size_t)LC_TRACKS * (g.ldo + g.ldk) + (2 * LC_TRACKS + 1) * (size_t)ms) * 4; }
inline size_t lin_lds_bwd(int D, int ms) { LinGeom g = lin_geom(D); return ((size_t)LC_TRACKS * (g.ldo + g.ldk) + (2 * LC_TRACKS + 3) * (size_t)ms) * 4; }

struct LinArgs {
  int D, n_panels, max_steps, act;
  const int32_t* panel; const int32_t* rows; const int32_t* sinfo;
  const float* dt;
  float lambda;
  const float4* wf[TEMP_CHAIN_MAX_RNN];      // forward pieces of every W
  const float4* wb[TEMP_CHAIN_MAX_RNN];      // backward pieces
};
struct LinUps { int n; const float* p[TEMP_CHAIN_MAX_UP]; };
struct LinPackJobs { int count; const float* w[TEMP_CHAIN_MAX_RNN]; float4* out[TEMP_CHAIN_MAX_RNN]; };

// ---- W (in, out) -> fragment order -----------------------------------------------------------------------------------
// forward  piece (tile, q, lane): float4 e -> W[8q + 4hh + e][tile*32 + li]      (k = input column, n = output column)
// backward piece (tile, q, lane): float4 e -> W[tile*32 + li][8q + 4hh + e]      (n = input column, k = output column)
// zero outside the matrix.  li = lane & 31, hh = lane >> 5: the A-operand layout of v_mfma_f32_32x32x2_f32 (lane supplies
// A[i = li][k = hh]); one float4 feeds 4 consecutive MFMAs, the B fragment is read in the same k order.  blockIdx.y = the matrix.
__global__ void __launch_bounds__(256) k_lin_chain_pack(int D, LinPackJobs jobs) {
  const LinGeom g = lin_geom(D);
  const float* __restrict__ W = jobs.w[blockIdx.y];
  float4* __restrict__ out = jobs.out[blockIdx.y];
  const int half = g.NT * g.NQ * 64;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < 2 * half; i += gridDim.x * blockDim.x) {
    const bool fwd = i < half;
    const int j = fwd ? i : i - half;
    const int lane = j & 63, rest = j >> 6;
    const int tile = rest / g.NQ, q = rest - tile * g.NQ;
    const int n = tile * 32 + (lane & 31), k = 8 * q + 4 * (lane >> 5);
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const bool in = n < D && k + e < D;
      v[e] = !in ? 0.f : fwd ? W[(size_t)(k + e) * D + n] : W[(size_t)n * D + k + e];
    }
    out[i] = make_float4(v[0], v[1], v[2], v[3]);
  }
}

// out[track][tile*32 ..] = sum_s sum_k piece_s(tile, k) . kb_s[track][k] for the wave's tiles (wave, wave + 4): two independent
// accumulators; the NS sources (weight, B operand) are walked one behind the other into the same accumulators (a K = NS d product)
template <int NS>
__device__ __forceinline__ void lin_product_n(const float4* const (&w)[NS], const float* const (&kb)[NS], float* ob, const LinGeom& g, int wave, int lane) {
  const int li = lane & 31, hh = lane >> 5;
  for (int t0 = wave; t0 < g.NT; t0 += 8) {
    const int t1 = t0 + 4;
    const bool two = t1 < g.NT;
    f32x16 a0, a1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { a0[r] = 0.f; a1[r] = 0.f; }
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const float* krow = kb[s] + li * g.ldk + 4 * hh;
      const float4* w0 = w[s] + (size_t)t0 * g.NQ * 64 + lane;
      const float4* w1 = w[s] + (size_t)(two ? t1 : t0) * g.NQ * 64 + lane;
#pragma unroll 2
      for (int q = 0; q < g.NQ; ++q) {
        const float4 x0 = w0[(size_t)q * 64], x1 = w1[(size_t)q * 64];
        const float4 h4 = ld4(krow + 8 * q);
        a0 = __builtin_amdgcn_mfma_f32_32x32x2f32(x0.x, h4.x, a0, 0, 0, 0);
        a1 = __builtin_amdgcn_mfma_f32_32x32x2f32(x1.x, h4.x, a1, 0, 0, 0);
        a0 = __builtin_amdgcn_mfma_f32_32x32x2f32(x0.y, h4.y, a0, 0, 0, 0);
        a1 = __builtin_amdgcn_mfma_f32_32x32x2f32(x1.y, h4.y, a1, 0, 0, 0);
        a0 = __builtin_amdgcn_mfma_f32_32x32x2f32(x0.z, h4.z, a0, 0, 0, 0);
        a1 = __builtin_amdgcn_mfma_f32_32x32x2f32(x1.z, h4.z, a1, 0, 0, 0);
        a0 = __builtin_amdgcn_mfma_f32_32x32x2f32(x0.w, h4.w, a0, 0, 0, 0);
        a1 = __builtin_amdgcn_mfma_f32_32x32x2f32(x1.w, h4.w, a1, 0, 0, 0);
      }
    }
    // lane (li, hh) owns track li and, per register quad qq, columns tile*32 + 8qq + 4hh .. +3
    float* d0 = ob + li * g.ldo + t0 * 32 + 4 * hh;
#pragma unroll
    for (int qq = 0; qq < 4; ++qq) st4(d0 + 8 * qq, make_float4(a0[4 * qq], a0[4 * qq + 1], a0[4 * qq + 2], a0[4 * qq + 3]));
    if (two) {
      float* d1 = ob + li * g.ldo + t1 * 32 + 4 * hh;
#pragma unroll
      for (int qq = 0; qq < 4; ++qq) st4(d1 + 8 * qq, make_float4(a1[4 * qq], a1[4 * qq + 1], a1[4 * qq + 2], a1[4 * qq + 3]));
    }
  }
}

__device__ __forceinline__ void lin_product(const float4* __restrict__ w, const float* kb, float* ob, const LinGeom& g, int wave, int lane) {
  const float4* const ws[1] = {w};
  const float* const ks[1] = {kb};
  lin_product_n<1>(ws, ks, ob, g, wave, lane);
}

__device__ __forceinline__ float4 relu4(float4 v) { return make_float4(fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f)); }

// ---- forward ----------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(LC_THREADS) k_lin_chain_fwd(LinArgs a, const float* __restrict__ x, const int32_t* __restrict__ x_index,
                                                              float* __restrict__ H, float* __restrict__ HD) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int D = a.D, D4 = D >> 2;
  const LinGeom g = lin_geom(D);
  float* sb = lds;                                          // [32][ldo] the tracks' states; raw products between phases 2 and 3
  float* kb = sb + LC_TRACKS * g.ldo;                       // [32][ldk] decayed states of the step (B operand)
  int* tabb = (int*)(kb + LC_TRACKS * g.ldk);               // [ms][32] the panel's row table
  float* decb = (float*)(tabb + LC_TRACKS * a.max_steps);   // [ms][32] decay factor of every row
  int* flagb = (int*)(decb + LC_TRACKS * a.max_steps);      // [ms] step flags
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int items = LC_TRACKS * D4;

  for (int p = blockIdx.x; p < a.n_panels; p += gridDim.x) {
    const int wi = a.panel[4 * p], s0 = a.panel[4 * p + 1], ns = a.panel[4 * p + 2];
    __syncthreads();                                        // (the panel before this one is done with the tables)
    for (int i = tid; i < LC_TRACKS * g.ldk; i += LC_THREADS) kb[i] = 0.f;        // the k padding must be 0, not stale LDS
    for (int i = tid; i < ns * LC_TRACKS; i += LC_THREADS) {
      const int e = a.rows[(size_t)s0 * LC_TRACKS + i];
      tabb[i] = e;
      decb[i] = e >= 0 ? expf(-a.dt[e & LC_ROW_MASK] * a.lambda) : 0.f;
    }
    for (int i = tid; i < ns; i += LC_THREADS) flagb[i] = a.sinfo[4 * (size_t)(s0 + i)];
    __syncthreads();

    for (int s = 0; s < ns; ++s) {
      const bool any_prev = (flagb[s] & 1) != 0;
      // 1: hdec = dec . (the track's state), 0 for a row without a previous state (a select: stale LDS is never multiplied)
      for (int i = tid; i < items; i += LC_THREADS) {
        const int t = i / D4, c = (i - t * D4) << 2;
        const int e = tabb[s * LC_TRACKS + t];
        float4 hd = zero4();
        if (e >= 0) {
          if (e & LC_HAS_PREV) hd = scale4(ld4(sb + t * g.ldo + c), decb[s * LC_TRACKS + t]);
          st4(HD + (size_t)(e & LC_ROW_MASK) * D + c, hd);
        }
        st4(kb + t * g.ldk + c, hd);
      }
      __syncthreads();
      // 2: hdec . W (skipped where no track of the step carries a state: the product is 0)
      if (any_prev) lin_product(a.wf[wi], kb, sb, g, wave, lane);
      __syncthreads();
      // 3: h = act(x + product)
      for (int i = tid; i < items; i += LC_THREADS) {
        const int t = i / D4, c = (i - t * D4) << 2;
        const int e = tabb[s * LC_TRACKS + t];
        if (e < 0) continue;
        const int row = e & LC_ROW_MASK;
        const size_t xr = x_index ? (size_t)x_index[row] : (size_t)row;
        float4 v = ld4(x + xr * D + c);
        if (any_prev) v = add4(v, ld4(sb + t * g.ldo + c));
        if (a.act) v = relu4(v);
        st4(H + (size_t)row * D + c, v);
        st4(sb + t * g.ldo + c, v);
      }
    }
  }
}

// ---- backward ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(LC_THREADS) k_lin_chain_bwd(LinArgs a, LinUps ups, const float* __restrict__ H, float* __restrict__ DP) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int D = a.D, D4 = D >> 2;
  const LinGeom g = lin_geom(D);
  float* pb = lds;                                          // [32][ldo] raw d_pre . W^T of the step walked before (the successor's)
  float* kb = pb + LC_TRACKS * g.ldo;                       // [32][ldk] d_pre of the step (B operand)
  int* tabb = (int*)(kb + LC_TRACKS * g.ldk);
  float* decb = (float*)(tabb + LC_TRACKS * a.max_steps);
  int* infob = (int*)(decb + LC_TRACKS * a.max_steps);      // [ms][3] flags, up, up_row0
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int items = LC_TRACKS * D4;

  for (int p = blockIdx.x; p < a.n_panels; p += gridDim.x) {
    const int wi = a.panel[4 * p], s0 = a.panel[4 * p + 1], ns = a.panel[4 * p + 2];
    __syncthreads();
    for (int i = tid; i < LC_TRACKS * g.ldk; i += LC_THREADS) kb[i] = 0.f;
    for (int i = tid; i < ns * LC_TRACKS; i += LC_THREADS) {
      const int e = a.rows[(size_t)s0 * LC_TRACKS + i];
      tabb[i] = e;
      decb[i] = e >= 0 ? expf(-a.dt[e & LC_ROW_MASK] * a.lambda) : 0.f;
    }
    for (int i = tid; i < 3 * ns; i += LC_THREADS) { const int s = i / 3; infob[i] = a.sinfo[4 * (size_t)(s0 + s) + (i - 3 * s)]; }
    __syncthreads();

    for (int s = ns - 1; s >= 0; --s) {
      const int flags = infob[3 * s], up = infob[3 * s + 1], up0 = infob[3 * s + 2];
      const float* upp = ((flags & 2) && up >= 0 && up < ups.n) ? ups.p[up] : nullptr;
      const bool succ = s + 1 < ns;
      // 1: g = upstream + dec(successor) . d_prev(successor);  d_pre = g . [h > 0]
      for (int i = tid; i < items; i += LC_THREADS) {
        const int t = i / D4, c = (i - t * D4) << 2;
        const int e = tabb[s * LC_TRACKS + t];
        float4 gv = zero4();
        if (e >= 0) {
          const int row = e & LC_ROW_MASK;
          if (upp) gv = ld4(upp + (size_t)(row - up0) * D + c);
          if (succ) {
            const int en = tabb[(s + 1) * LC_TRACKS + t];
            if (en >= 0 && (en & LC_HAS_PREV)) gv = fma4(decb[(s + 1) * LC_TRACKS + t], ld4(pb + t * g.ldo + c), gv);
          }
          if (a.act) gv = relu_gate4(ld4(H + (size_t)row * D + c), gv);
          st4(DP + (size_t)row * D + c, gv);
        }
        st4(kb + t * g.ldk + c, gv);
      }
      __syncthreads();
      // 2: d_pre . W^T, read by the step before this one (only rows with a previous state hand a gradient back)
      if (flags & 1) lin_product(a.wb[wi], kb, pb, g, wave, lane);
      __syncthreads();
    }
  }
}

// ---- one position on gathered rows, NS history sources in front of one activation (temp_lin_rows_* NS = 1, temp_lin_rows2_* NS = 2) ----
// NS = 1: the pair rows of the batched all-entity pass, one step of the chain without the track tables.  NS = 2: BiRRGCNLayer's
// centre / isolated form, where the activation follows the SUM of both directions' recurrent terms, so the two sources of a row go
// through one kernel.  A workgroup owns rows 32 b .. 32 b + 31 and runs the three phases once; a row past n is a zero row of the B
// operand and is never stored.  Forward: the NS decayed tiles lie in LDS side by side and the product walks [hdec_0 | .. ] against
// [W_0 ; ..] into one accumulator set (K = NS d), source 0 first.  Backward: the one d_pre tile against every W_s^T into NS product
// tiles.  LDS: 32 (ldo + NS ldk) words forward, 32 (NS ldo + ldk) backward, + 64 NS for the tables.  NS = 1: 55 552 / 66 816 bytes at
// d = 200 / 256; NS = 2: 81 920 / 84 992 at d = 200, 100 352 at d = 256 (of the 160 KB a workgroup has).
#define LR_ROWS LC_TRACKS
template <int NS>
struct LinRows {                                             // per source (NS = 2: index 0 forward direction, 1 backward direction)
  const float* H[NS]; const int32_t* rows[NS]; const float* dt[NS];      // (H is not read by the backward)
  const float4* w[NS];                                       // the forward (fwd kernel) / backward (bwd kernel) piece of W_s
  float* o[NS];                                              // hdec_s (fwd kernel) / d_hrows_s (bwd kernel)
};
inline size_t lin_lds_rows_fwd(int D, int NS) { LinGeom g = lin_geom(D); return ((size_t)LR_ROWS * (g.ldo + NS * g.ldk) + 2 * NS * LR_ROWS) * 4; }
inline size_t lin_lds_rows_bwd(int D, int NS) { LinGeom g = lin_geom(D); return ((size_t)LR_ROWS * (NS * g.ldo + g.ldk) + 2 * NS * LR_ROWS) * 4; }

// hrb[s][t] = the H row of row t in source s (-1: none, or past n), decb[s][t] its decay factor: threads 0 .. 32 NS - 1
template <int NS>
__device__ __forceinline__ void lin_rows_tables(const LinRows<NS>& a, int n, long long row0, float lambda, int* hrb, float* decb, int tid) {
  if (tid < NS * LR_ROWS) {
    const long long row = row0 + (tid & (LR_ROWS - 1));
    const int32_t* rows = a.rows[0];
    const float* dt = a.dt[0];
#pragma unroll
    for (int s = 1; s < NS; ++s)
      if (tid >= s * LR_ROWS) { rows = a.rows[s]; dt = a.dt[s]; }
    const int hr = row < n ? rows[row] : -1;
    hrb[tid] = hr;
    decb[tid] = hr >= 0 ? expf(-dt[row] * lambda) : 0.f;
  }
}

template <int NS>
__global__ void __launch_bounds__(LC_THREADS) k_lin_rows_fwd(int n, int D, int act, float lambda, LinRows<NS> a, const float* __restrict__ x,
                                                             const int32_t* __restrict__ x_rows, float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int D4 = D >> 2;
  const LinGeom g = lin_geom(D);
  float* sb = lds;                                          // [32][ldo] raw products
  float* kb = sb + LR_ROWS * g.ldo;                         // [NS][32][ldk] decayed rows of every source (B operands)
  int* hrb = (int*)(kb + NS * LR_ROWS * g.ldk);             // [NS][32]
  float* decb = (float*)(hrb + NS * LR_ROWS);               // [NS][32]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int items = LR_ROWS * D4;
  const long long row0 = (long long)blockIdx.x * LR_ROWS;

  for (int i = tid; i < NS * LR_ROWS * g.ldk; i += LC_THREADS) kb[i] = 0.f;       // the k padding must be 0, not stale LDS
  lin_rows_tables<NS>(a, n, row0, lambda, hrb, decb, tid);
  __syncthreads();
  // 1: hdec_s = dec_s . H_s[rows_s], 0 for a row without a previous state in that source
  const float* ks[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const float* __restrict__ H = a.H[s];
    float* __restrict__ HD = a.o[s];
    float* k = kb + s * LR_ROWS * g.ldk;
    ks[s] = k;
    for (int i = tid; i < items; i += LC_THREADS) {
      const int t = i / D4, c = (i - t * D4) << 2;
      const long long row = row0 + t;
      const int hr = hrb[s * LR_ROWS + t];
      float4 hd = zero4();
      if (hr >= 0) hd = scale4(ld4(H + (size_t)hr * D + c), decb[s * LR_ROWS + t]);
      if (row < n) st4(HD + (size_t)row * D + c, hd);
      st4(k + t * g.ldk + c, hd);
    }
  }
  __syncthreads();
  // 2: [hdec_0 | ..] . [W_0 ; ..]
  lin_product_n<NS>(a.w, ks, sb, g, wave, lane);
  __syncthreads();
  // 3: out = act(x + product)
  for (int i = tid; i < items; i += LC_THREADS) {
    const int t = i / D4, c = (i - t * D4) << 2;
    const long long row = row0 + t;
    if (row >= n) continue;
    const long long xr = x_rows ? (long long)x_rows[row] : row;
    float4 v = ld4(sb + t * g.ldo + c);
    if (xr >= 0) v = add4(v, ld4(x + (size_t)xr * D + c));
    if (act) v = relu4(v);
    st4(out + (size_t)row * D + c, v);
  }
}

template <int NS>
__global__ void __launch_bounds__(LC_THREADS) k_lin_rows_bwd(int n, int D, int act, float lambda, LinRows<NS> a, const float* __restrict__ out,
                                                             const float* __restrict__ up, float* __restrict__ DP) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int D4 = D >> 2;
  const LinGeom g = lin_geom(D);
  float* pb = lds;                                          // [NS][32][ldo] raw d_pre . W_s^T
  float* kb = pb + NS * LR_ROWS * g.ldo;                    // [32][ldk] d_pre (B operand of every product)
  int* hrb = (int*)(kb + LR_ROWS * g.ldk);
  float* decb = (float*)(hrb + NS * LR_ROWS);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int items = LR_ROWS * D4;
  const long long row0 = (long long)blockIdx.x * LR_ROWS;

  for (int i = tid; i < LR_ROWS * g.ldk; i += LC_THREADS) kb[i] = 0.f;
  lin_rows_tables<NS>(a, n, row0, lambda, hrb, decb, tid);
  __syncthreads();
  // 1: d_pre = upstream . [out > 0]
  for (int i = tid; i < items; i += LC_THREADS) {
    const int t = i / D4, c = (i - t * D4) << 2;
    const long long row = row0 + t;
    float4 gv = zero4();
    if (row < n) {
      gv = ld4(up + (size_t)row * D + c);
      if (act) gv = relu_gate4(ld4(out + (size_t)row * D + c), gv);
      st4(DP + (size_t)row * D + c, gv);
    }
    st4(kb + t * g.ldk + c, gv);
  }
  __syncthreads();
  // 2: d_pre . W_s^T (one B operand, NS product tiles: no barrier between them)
#pragma unroll
  for (int s = 0; s < NS; ++s) lin_product(a.w[s], kb, pb + s * LR_ROWS * g.ldo, g, wave, lane);
  __syncthreads();
  // 3: d_hrows_s = dec_s . product_s, 0 for a row without a previous state in that source (a select: the product of such a row is not read)
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    float* __restrict__ DH = a.o[s];
    const float* ps = pb + s * LR_ROWS * g.ldo;
    for (int i = tid; i < items; i += LC_THREADS) {
      const int t = i / D4, c = (i - t * D4) << 2;
      const long long row = row0 + t;
      if (row >= n) continue;
      st4(DH + (size_t)row * D + c, hrb[s * LR_ROWS + t] >= 0 ? scale4(ld4(ps + t * g.ldo + c), decb[s * LR_ROWS + t]) : zero4());
    }
  }
}

template <class K>
static int lin_lds_attr(K kernel, bool* done) {
  if (*done) return TEMP_OK;
  if (hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, LC_LDS_LIMIT) != hipSuccess) return TEMP_E_LAUNCH;
  *done = true;
  return TEMP_OK;
}

static std::atomic<long long> g_lin_launches{0};

}  // namespace temp

using namespace temp;

extern "C" {

int temp_lin_chain_supported(int d, int max_steps) {
  if (d <= 0 || d % 4 || d > TEMP_CHAIN_MAX_D || max_steps < 0 || max_steps > LC_MAX_STEPS) return 0;
  return lin_lds_fwd(d, LC_MAX_STEPS) <= LC_LDS_LIMIT && lin_lds_bwd(d, LC_MAX_STEPS) <= LC_LDS_LIMIT;
}

size_t temp_lin_chain_pack_floats(int d) {
  if (d <= 0) return 0;
  const LinGeom g = lin_geom(d);
  return (size_t)2 * g.NT * g.NQ * 64 * 4;
}

int temp_lin_chain_pack_multi(int count, int d, const float* const* w, float* const* packed, void* stream) {
  if (count <= 0 || count > TEMP_CHAIN_MAX_RNN || d <= 0 || !w || !packed) return TEMP_E_BADARG;
  for (int i = 0; i < count; ++i) if (!w[i] || !packed[i]) return TEMP_E_BADARG;
  if (!temp_lin_chain_supported(d, 0)) return TEMP_E_UNSUPPORTED;
  const LinGeom g = lin_geom(d);
  LinPackJobs jobs = {};
  jobs.count = count;
  for (int i = 0; i < count; ++i) { jobs.w[i] = w[i]; jobs.out[i] = (float4*)packed[i]; }
  TEMP_LAUNCH(K_LIN_CHAIN_PACK, k_lin_chain_pack, dim3(ceil_div((long long)2 * g.NT * g.NQ * 64, 256), count), dim3(256), 0, (hipStream_t)stream, d, jobs);
  return launch_status();
}

}  // extern "C"

// descriptor checks shared by both calls; *launch = 0 where the call succeeds without one (no panels)
static int lin_check(const TempLinChain* c, LinArgs* a, int* launch) {
  *launch = 0;
  if (!c || c->d <= 0 || c->n_panels < 0 || c->n_steps < 0 || c->max_steps < 0) return TEMP_E_BADARG;
  if (c->n_w < 1 || c->n_w > TEMP_CHAIN_MAX_RNN || (c->act != 0 && c->act != 1)) return TEMP_E_BADARG;
  for (int i = 0; i < c->n_w; ++i) if (!c->packed[i]) return TEMP_E_BADARG;
  if (c->n_panels > 0 && (!c->panel || !c->rows || !c->sinfo || !c->dt || c->max_steps == 0)) return TEMP_E_BADARG;
  if (!temp_lin_chain_supported(c->d, c->max_steps)) return TEMP_E_UNSUPPORTED;
  if (c->n_panels == 0) return TEMP_OK;
  const LinGeom g = lin_geom(c->d);
  LinArgs r = {};
  r.D = c->d; r.n_panels = c->n_panels; r.max_steps = c->max_steps; r.act = c->act;
  r.panel = c->panel; r.rows = c->rows; r.sinfo = c->sinfo; r.dt = c->dt; r.lambda = c->lambda;
  for (int i = 0; i < c->n_w; ++i) {
    r.wf[i] = (const float4*)c->packed[i];
    r.wb[i] = r.wf[i] + (size_t)g.NT * g.NQ * 64;
  }
  *a = r;
  *launch = 1;
  return TEMP_OK;
}

extern "C" {

int temp_lin_chain_fwd(const TempLinChain* c, const float* x, const int32_t* x_index, float* h, float* hdec, void* stream) {
  LinArgs a;
  int launch;
  const int rc = lin_check(c, &a, &launch);
  if (rc || !launch) return rc;
  if (!x || !h || !hdec) return TEMP_E_BADARG;
  static bool attr = false;
  if (lin_lds_attr(k_lin_chain_fwd, &attr)) return TEMP_E_LAUNCH;
  g_lin_launches.fetch_add(1, std::memory_order_relaxed);
  TEMP_LAUNCH(K_LIN_CHAIN_FWD, k_lin_chain_fwd, dim3(a.n_panels), dim3(LC_THREADS), lin_lds_fwd(a.D, a.max_steps), (hipStream_t)stream, a, x, x_index, h, hdec);
  return launch_status();
}

int temp_lin_chain_bwd(const TempLinChain* c, const float* h, int32_t n_up, const float* const* up, float* d_pre, void* stream) {
  LinArgs a;
  int launch;
  const int rc = lin_check(c, &a, &launch);
  if (rc) return rc;
  if (n_up < 0 || n_up > TEMP_CHAIN_MAX_UP || (n_up > 0 && !up)) return TEMP_E_BADARG;
  if (!launch) return TEMP_OK;
  if (!h || !d_pre) return TEMP_E_BADARG;
  LinUps ups = {};
  ups.n = n_up;
  for (int i = 0; i < n_up; ++i) ups.p[i] = up[i];
  static bool attr = false;
  if (lin_lds_attr(k_lin_chain_bwd, &attr)) return TEMP_E_LAUNCH;
  g_lin_launches.fetch_add(1, std::memory_order_relaxed);
  TEMP_LAUNCH(K_LIN_CHAIN_BWD, k_lin_chain_bwd, dim3(a.n_panels), dim3(LC_THREADS), lin_lds_bwd(a.D, a.max_steps), (hipStream_t)stream, a, ups, h, d_pre);
  return launch_status();
}

long long temp_lin_chain_launches(void) { return g_lin_launches.load(std::memory_order_relaxed); }

}  // extern "C"

static int lin_rows_supported(int d, int ns) {
  return temp_lin_chain_supported(d, 0) && lin_lds_rows_fwd(d, ns) <= LC_LDS_LIMIT && lin_lds_rows_bwd(d, ns) <= LC_LDS_LIMIT;
}

// The body of the four temp_lin_rows*_fwd / _bwd calls.  FWD: p0 = x, p1 = x_rows (int32, may be null), p2 = out; else p0 = out (may be
// null without the activation), p1 = up, p2 = d_pre.
template <int NS, bool FWD>
static int lin_rows_run(int n, int d, int act, float lambda, const LinRows<NS>& a, const float* p0, const void* p1, float* p2, void* stream) {
  if (n < 0 || d <= 0 || (act != 0 && act != 1)) return TEMP_E_BADARG;
  if (!lin_rows_supported(d, NS)) return TEMP_E_UNSUPPORTED;
  if (n == 0) return TEMP_OK;
  bool ok = p2 && (FWD ? p0 != nullptr : p1 && (p0 || !act));
  for (int s = 0; s < NS; ++s) ok = ok && (a.H[s] || !FWD) && a.rows[s] && a.dt[s] && a.w[s] && a.o[s];
  if (!ok) return TEMP_E_BADARG;
  static bool attr = false;                                  // (one per instantiation = per kernel)
  const dim3 grid(ceil_div(n, LR_ROWS)), block(LC_THREADS);
  if constexpr (FWD) {
    if (lin_lds_attr(k_lin_rows_fwd<NS>, &attr)) return TEMP_E_LAUNCH;
    TEMP_LAUNCH(NS == 1 ? K_LIN_ROWS_FWD : K_LIN_ROWS2_FWD, k_lin_rows_fwd<NS>, grid, block, lin_lds_rows_fwd(d, NS), (hipStream_t)stream, n, d, act, lambda,
                a, p0, (const int32_t*)p1, p2);
  } else {
    if (lin_lds_attr(k_lin_rows_bwd<NS>, &attr)) return TEMP_E_LAUNCH;
    TEMP_LAUNCH(NS == 1 ? K_LIN_ROWS_BWD : K_LIN_ROWS2_BWD, k_lin_rows_bwd<NS>, grid, block, lin_lds_rows_bwd(d, NS), (hipStream_t)stream, n, d, act, lambda,
                a, p0, (const float*)p1, p2);
  }
  return launch_status();
}

extern "C" {

int temp_lin_rows_supported(int d) { return lin_rows_supported(d, 1); }
int temp_lin_rows2_supported(int d) { return lin_rows_supported(d, 2); }

int temp_lin_rows_fwd(int n, int d, const float* x, const int32_t* x_rows, const float* H, const int32_t* h_rows, const float* dt, float lambda,
                      const float* pack_fwd, int act, float* out, float* hdec, void* stream) {
  const LinRows<1> a = {{H}, {h_rows}, {dt}, {(const float4*)pack_fwd}, {hdec}};
  return lin_rows_run<1, true>(n, d, act, lambda, a, x, x_rows, out, stream);
}

int temp_lin_rows_bwd(int n, int d, const float* out, const float* up, const int32_t* h_rows, const float* dt, float lambda, const float* pack_bwd,
                      int act, float* d_pre, float* d_hrows, void* stream) {
  const LinRows<1> a = {{nullptr}, {h_rows}, {dt}, {(const float4*)pack_bwd}, {d_hrows}};
  return lin_rows_run<1, false>(n, d, act, lambda, a, out, up, d_pre, stream);
}

int temp_lin_rows2_fwd(int n, int d, const float* x, const int32_t* x_rows, const float* H_f, const int32_t* rows_f, const float* dt_f,
                       const float* H_b, const int32_t* rows_b, const float* dt_b, float lambda, const float* pack_fwd_f, const float* pack_fwd_b,
                       int act, float* out, float* hdec_f, float* hdec_b, void* stream) {
  const LinRows<2> a = {{H_f, H_b}, {rows_f, rows_b}, {dt_f, dt_b}, {(const float4*)pack_fwd_f, (const float4*)pack_fwd_b}, {hdec_f, hdec_b}};
  return lin_rows_run<2, true>(n, d, act, lambda, a, x, x_rows, out, stream);
}

int temp_lin_rows2_bwd(int n, int d, const float* out, const float* up, const int32_t* rows_f, const float* dt_f, const int32_t* rows_b,
                       const float* dt_b, float lambda, const float* pack_bwd_f, const float* pack_bwd_b, int act, float* d_pre, float* d_hrows_f,
                       float* d_hrows_b, void* stream) {
  const LinRows<2> a = {{nullptr, nullptr}, {rows_f, rows_b}, {dt_f, dt_b}, {(const float4*)pack_bwd_f, (const float4*)pack_bwd_b}, {d_hrows_f, d_hrows_b}};
  return lin_rows_run<2, false>(n, d, act, lambda, a, out, up, d_pre, stream);
}

}  // extern "C"
