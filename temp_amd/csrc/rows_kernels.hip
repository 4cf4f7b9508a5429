// Row gather, atomic scatter-add and the deterministic segment sums (the adjoint of a row gather whose index list is known in
// advance), with their entry points.
#include "common.hpp"
#include "hx_pack.hpp"

namespace temp {

__global__ void __launch_bounds__(256) k_gather_rows(int n, int d4, const float4* __restrict__ table, const int32_t* __restrict__ idx,
                                                     float4* __restrict__ out) {
  const size_t total = (size_t)n * d4;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int r = (int)(i / d4), c = (int)(i - (size_t)r * d4);
    const int s = idx[r];
    out[i] = (s >= 0) ? table[(size_t)s * d4 + c] : zero4();
  }
}

__global__ void __launch_bounds__(256) k_scatter_add_rows(int n, int d, const float* __restrict__ src, const int32_t* __restrict__ idx,
                                                          float* __restrict__ table) {
  const size_t total = (size_t)n * d;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int r = (int)(i / d), c = (int)(i - (size_t)r * d);
    const int s = idx[r];
    if (s >= 0) atomicAdd(table + (size_t)s * d + c, src[i]);
  }
}

// out[s] = sum over j in [seg_ptr[s], seg_ptr[s+1]) of src[order[j]]  -- the adjoint of a row gather whose index
// list is known in advance (its inverse, grouped by table row, is built once on the host).  Deterministic
// replacement of the atomic scatter for hot tables: GDELT has 500 entities and ~100 k gathered rows per step,
// i.e. ~200 atomic adds per table element.  One wave per segment, one float4 per lane, 4 row loads in flight;
// the d/4-lane groups of a wave (LPR lanes each) take every (64/LPR)-th row and are summed by shuffles.
// WIDE (d4 > 64, LPR = 64): the wave walks the segment once per 64 float4 columns.
template <int LPR, bool WIDE = false>
__global__ void __launch_bounds__(256) k_segment_sum_rows(int n_seg, int d4, const int32_t* __restrict__ seg_ptr,
                                                          const int32_t* __restrict__ order, const float4* __restrict__ src,
                                                          const int32_t* __restrict__ row_mask, const float4* __restrict__ relu_of,
                                                          float4* __restrict__ out) {
  constexpr int G = 64 / LPR;
  static_assert(!WIDE || LPR == 64, "the column loop is for rows wider than a wave");
  const int lane = threadIdx.x & 63, grp = lane / LPR, lr0 = lane - grp * LPR;
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = (gridDim.x * blockDim.x) >> 6;
  for (int s = wave; s < n_seg; s += nwaves) {
    const int beg = seg_ptr[s], end = seg_ptr[s + 1];
    for (int c0 = 0; c0 < (WIDE ? d4 : 1); c0 += LPR) {                   // (one trip unless WIDE)
      const int lr = c0 + lr0;
      const bool col_ok = lr < d4;
      float4 acc = zero4();
      int j = beg + grp;
      for (; j + 3 * G < end; j += 4 * G) {
        const int r0 = order[j], r1 = order[j + G], r2 = order[j + 2 * G], r3 = order[j + 3 * G];
        const bool m0 = !row_mask || row_mask[r0] > 0, m1 = !row_mask || row_mask[r1] > 0, m2 = !row_mask || row_mask[r2] > 0,
                   m3 = !row_mask || row_mask[r3] > 0;          // masked rows were never written by their producer
        float4 v0 = zero4(), v1 = zero4(), v2 = zero4(), v3 = zero4();
        if (col_ok) {
          if (m0) v0 = src[(size_t)r0 * d4 + lr];
          if (m1) v1 = src[(size_t)r1 * d4 + lr];
          if (m2) v2 = src[(size_t)r2 * d4 + lr];
          if (m3) v3 = src[(size_t)r3 * d4 + lr];
        }
        acc = add4(add4(acc, v0), add4(v1, add4(v2, v3)));
      }
      for (; j < end; j += G) {
        const int r = order[j];
        if (col_ok && (!row_mask || row_mask[r] > 0)) acc = add4(acc, src[(size_t)r * d4 + lr]);
      }
#pragma unroll
      for (int m = LPR; m < 64; m <<= 1) acc = add4(acc, shfl_xor4(acc, m));
      if (grp == 0 && col_ok) out[(size_t)s * d4 + lr] = relu_of ? relu_gate4(relu_of[(size_t)s * d4 + lr], acc) : acc;
    }
  }
}

// The same for segments of one or two rows (the adjoint of a gather whose rows are mostly distinct).
template <int LPR, bool WIDE = false>
__global__ void __launch_bounds__(256) k_segment_sum_rows_short(int n_seg, int d4, const int32_t* __restrict__ seg_ptr,
                                                          const int32_t* __restrict__ order, const float4* __restrict__ src,
                                                          const int32_t* __restrict__ row_mask, const float4* __restrict__ relu_of,
                                                          float4* __restrict__ out) {
  // A wave takes FOUR consecutive segments at a time and walks them in lockstep: the three dependent round trips of a segment
  // (seg_ptr -> order -> row) are then shared by four segments instead of paid by each (the gather adjoints have 1-2 rows per
  // segment: the walk is all latency).
  constexpr int G = 64 / LPR, U = 4;
  static_assert(!WIDE || LPR == 64, "the column loop is for rows wider than a wave");
  const int lane = threadIdx.x & 63, grp = lane / LPR, lr0 = lane - grp * LPR;
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = (gridDim.x * blockDim.x) >> 6;
  for (int s0 = wave * U; s0 < n_seg; s0 += nwaves * U) {
    int beg[U], len[U], maxlen = 0;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bool ok = s0 + u < n_seg;
      beg[u] = ok ? seg_ptr[s0 + u] : 0;
      len[u] = ok ? seg_ptr[s0 + u + 1] - beg[u] : 0;
      maxlen = max(maxlen, len[u]);
    }
    for (int c0 = 0; c0 < (WIDE ? d4 : 1); c0 += LPR) {                   // (one trip unless WIDE)
      const int lr = c0 + lr0;
      const bool col_ok = lr < d4;
      float4 acc[U];
#pragma unroll
      for (int u = 0; u < U; ++u) acc[u] = zero4();
      for (int k = grp; k < maxlen; k += G) {
        int r[U];
#pragma unroll
        for (int u = 0; u < U; ++u) r[u] = k < len[u] ? order[beg[u] + k] : -1;
        float4 v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          v[u] = zero4();
          if (r[u] >= 0 && col_ok && (!row_mask || row_mask[r[u]] > 0)) v[u] = src[(size_t)r[u] * d4 + lr];   // masked rows were never written
        }
#pragma unroll
        for (int u = 0; u < U; ++u) acc[u] = add4(acc[u], v[u]);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
#pragma unroll
        for (int m = LPR; m < 64; m <<= 1) acc[u] = add4(acc[u], shfl_xor4(acc[u], m));
        if (grp == 0 && col_ok && s0 + u < n_seg)
          out[(size_t)(s0 + u) * d4 + lr] = relu_of ? relu_gate4(relu_of[(size_t)(s0 + u) * d4 + lr], acc[u]) : acc[u];
      }
    }
  }
}

// Long segments (a hot table: hundreds of gathered rows per table row): one BLOCK per segment, its 4 waves take every
// 4th row with 8 row loads in flight each, partial sums meet in LDS in a fixed order.
template <int WAVES>
__global__ void __launch_bounds__(WAVES * 64) k_segment_sum_rows_blk(int n_seg, int d4, const int32_t* __restrict__ seg_ptr,
                                                                     const int32_t* __restrict__ order, const float4* __restrict__ src,
                                                                     const int32_t* __restrict__ row_mask, const float4* __restrict__ relu_of,
                                                                     float4* __restrict__ out) {
  // one block per segment: wave w takes rows w, w + WAVES, ... eight at a time; the waves' sums are added in wave order.
  // WAVES = 16 for segments of a hundred rows and more (500 entities gathered 82 000 times: 164 rows each -- four waves walk
  // them in five dependent round trips of order[] -> row, sixteen in two)
  __shared__ float4 red[WAVES][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool col_ok = lane < d4;
  for (int s = blockIdx.x; s < n_seg; s += gridDim.x) {
    const int beg = seg_ptr[s], end = seg_ptr[s + 1];
    float4 acc = zero4();
    for (int j0 = beg + wave; j0 < end; j0 += 8 * WAVES) {
      float4 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int j = j0 + WAVES * u;
        v[u] = zero4();
        if (j < end && col_ok) {
          const int r = order[j];
          if (!row_mask || row_mask[r] > 0) v[u] = src[(size_t)r * d4 + lane];
        }
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) acc = add4(acc, v[u]);
    }
    red[wave][lane] = acc;
    __syncthreads();
    if (wave == 0 && col_ok) {
      float4 t = red[0][lane];
#pragma unroll
      for (int w = 1; w < WAVES; ++w) t = add4(t, red[w][lane]);
      out[(size_t)s * d4 + lane] = relu_of ? relu_gate4(relu_of[(size_t)s * d4 + lane], t) : t;
    }
    __syncthreads();
  }
}

// Two sources over the SAME segmentation in one launch (the table layer's backward sums the aggregation part of d_h and dz per
// table row: same inverse map, one walk of order[] instead of two; a stays masked by row_mask as in the single-source kernels).
template <int WAVES>
__global__ void __launch_bounds__(WAVES * 64) k_segment_sum_rows_blk2(int n_seg, int d4a, int d4b, const int32_t* __restrict__ seg_ptr,
                                                                      const int32_t* __restrict__ order, const float4* __restrict__ src_a,
                                                                      const int32_t* __restrict__ mask_a, const float4* __restrict__ src_b,
                                                                      float4* __restrict__ out_a, float4* __restrict__ out_b) {
  __shared__ float4 red[2][WAVES][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool a_ok = lane < d4a, b_ok = lane < d4b;
  for (int s = blockIdx.x; s < n_seg; s += gridDim.x) {
    const int beg = seg_ptr[s], end = seg_ptr[s + 1];
    float4 acc_a = zero4(), acc_b = zero4();
    for (int j0 = beg + wave; j0 < end; j0 += 4 * WAVES) {
      float4 va[4], vb[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int j = j0 + WAVES * u;
        va[u] = zero4(); vb[u] = zero4();
        if (j < end) {
          const int r = order[j];
          if (a_ok && (!mask_a || mask_a[r] > 0)) va[u] = src_a[(size_t)r * d4a + lane];
          if (b_ok) vb[u] = src_b[(size_t)r * d4b + lane];
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) { acc_a = add4(acc_a, va[u]); acc_b = add4(acc_b, vb[u]); }
    }
    red[0][wave][lane] = acc_a;
    red[1][wave][lane] = acc_b;
    __syncthreads();
    if (wave < 2) {
      const bool ok = wave == 0 ? a_ok : b_ok;
      if (ok) {
        float4 t = red[wave][0][lane];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) t = add4(t, red[wave][w][lane]);
        if (wave == 0) out_a[(size_t)s * d4a + lane] = t; else out_b[(size_t)s * d4b + lane] = t;
      }
    }
    __syncthreads();
  }
}

int segment_sum_rows2(int n_seg, const int32_t* seg_ptr, const int32_t* order, int d_a, const float* src_a, const int32_t* mask_a, float* out_a,
                      int d_b, const float* src_b, float* out_b, hipStream_t st, long long n_rows_hint) {
  if (d_a % 4 == 0 && d_b % 4 == 0 && d_a <= 256 && d_b <= 256 && n_rows_hint >= 96LL * n_seg) {
    TEMP_LAUNCH(K_SEGMENT_SUM, k_segment_sum_rows_blk2<16>, dim3(n_seg < 4096 ? n_seg : 4096), dim3(16 * 64), 0, st, n_seg, d_a / 4, d_b / 4, seg_ptr, order,
                (const float4*)src_a, mask_a, (const float4*)src_b, (float4*)out_a, (float4*)out_b);
    return launch_status();
  }
  int rc = segment_sum_rows(n_seg, d_a, seg_ptr, order, src_a, mask_a, out_a, st, n_rows_hint);
  if (rc) return rc;
  return segment_sum_rows(n_seg, d_b, seg_ptr, order, src_b, nullptr, out_b, st, n_rows_hint);
}

// Very long segments (a 40-row relation table gathered 48 000 times by the loss): every segment is cut into S equal
// parts, one block per part writes its partial sum into the workspace, a second kernel adds the S partials in order.
__global__ void __launch_bounds__(256) k_segment_sum_part(int S, int d4, const int32_t* __restrict__ seg_ptr, const int32_t* __restrict__ order,
                                                          const float4* __restrict__ src, const int32_t* __restrict__ row_mask,
                                                          float4* __restrict__ part) {
  __shared__ float4 red[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool col_ok = lane < d4;
  const int s = blockIdx.y, p = blockIdx.x;
  const int beg0 = seg_ptr[s], end0 = seg_ptr[s + 1];
  const int chunk = (end0 - beg0 + S - 1) / S;
  const int beg = beg0 + p * chunk, end = min(end0, beg + chunk);
  float4 acc = zero4();
  for (int j0 = beg + wave; j0 < end; j0 += 32) {
    float4 v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int j = j0 + 4 * u;
      v[u] = zero4();
      if (j < end && col_ok) {
        const int r = order[j];
        if (!row_mask || row_mask[r] > 0) v[u] = src[(size_t)r * d4 + lane];
      }
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) acc = add4(acc, v[u]);
  }
  red[wave][lane] = acc;
  __syncthreads();
  if (wave == 0 && col_ok) part[((size_t)s * S + p) * d4 + lane] = add4(add4(red[0][lane], red[1][lane]), add4(red[2][lane], red[3][lane]));
}

__global__ void __launch_bounds__(256) k_segment_sum_fin(int n_seg, int S, int d4, const float4* __restrict__ part, const float4* __restrict__ relu_of,
                                                         float4* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)n_seg * d4) return;
  const size_t s = i / d4, c = i - s * d4;
  float4 acc = zero4();
  for (int p = 0; p < S; ++p) acc = add4(acc, part[(s * S + p) * d4 + c]);
  out[i] = relu_of ? relu_gate4(relu_of[i], acc) : acc;
}

// Segment sum over FIXED PIECES of the row list (skewed segmentations: the adjoint of a gather of Zipf-distributed entity rows has
// a few segments of hundreds to thousands of rows among thousands of short ones, and a wave per segment takes as long as the
// longest).  Wave c sums the rows order[32 c .. 32 c + 32) segment by segment, in row order -- all 32 row loads are issued before
// the first addition: one memory round trip per piece -- a segment that lies inside the piece is written to `out`; the FIRST and
// the LAST segment of the piece, when they reach beyond it, go to part[c][0] / part[c][1].  k_segment_sum_pieces_fin then adds the
// pieces of every such segment in piece order (and zero-fills the empty segments): fixed pieces, fixed order => bit-repeatable.
// Lanes = float4 columns (d4 <= 64).
#define SEGSUM_PIECE 32
#define SEGSUM_PIECE_LOG2 5
__global__ void __launch_bounds__(256) k_segment_sum_pieces(int n_seg, int n_rows, int d4, const int32_t* __restrict__ seg_ptr,
                                                            const int32_t* __restrict__ order, const float4* __restrict__ src,
                                                            const int32_t* __restrict__ row_mask, const float4* __restrict__ relu_of,
                                                            float4* __restrict__ out, float4* __restrict__ part) {
  const int lane = threadIdx.x & 63;
  const int c = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int r0 = c * SEGSUM_PIECE;
  n_rows = min(n_rows, seg_ptr[n_seg]);                                    // (the rows there are: order[] holds exactly seg_ptr[n_seg])
  if (r0 >= n_rows) return;
  const int r1 = min(r0 + SEGSUM_PIECE, n_rows);
  const bool col_ok = lane < d4;
  const int col = col_ok ? lane : 0;
  int mine = (r0 + lane < r1) ? order[r0 + lane] : -1;
  if (row_mask && mine >= 0 && row_mask[mine] <= 0) mine = -1;             // masked rows were never written by their producer
  float4 v[SEGSUM_PIECE];
#pragma unroll
  for (int u = 0; u < SEGSUM_PIECE; ++u) {
    const int r = __builtin_amdgcn_readlane(mine, u);
    v[u] = r >= 0 ? src[(size_t)r * d4 + col] : zero4();
  }
  // the segment of row r0 (wave-uniform binary search: seg_ptr is non-decreasing)
  int lo = 0, hi = n_seg - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (seg_ptr[mid + 1] > r0) hi = mid; else lo = mid + 1;
  }
  int sg = lo, sb = seg_ptr[sg], se = seg_ptr[sg + 1];
  float4 acc = zero4();
  auto flush = [&]() {
    if (!col_ok) return;
    if (sb >= r0 && se <= r1) out[(size_t)sg * d4 + lane] = relu_of ? relu_gate4(relu_of[(size_t)sg * d4 + lane], acc) : acc;
    else part[((size_t)c * 2 + (sb <= r0 ? 0 : 1)) * d4 + lane] = acc;
  };
#pragma unroll
  for (int u = 0; u < SEGSUM_PIECE; ++u) {
    const int row = r0 + u;
    if (row < r1) {
      if (row == se) {                                                     // (wave-uniform) the next non-empty segment starts here
        flush();
        do { ++sg; se = seg_ptr[sg + 1]; } while (se <= row);
        sb = seg_ptr[sg];
        acc = zero4();
      }
      acc = add4(acc, v[u]);
    }
  }
  flush();
}

__global__ void __launch_bounds__(256) k_segment_sum_pieces_fin(int n_seg, int d4, const int32_t* __restrict__ seg_ptr, const float4* __restrict__ part,
                                                                const float4* __restrict__ relu_of, float4* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = (gridDim.x * blockDim.x) >> 6;
  const bool col_ok = lane < d4;
  for (int s = wave; s < n_seg; s += nwaves) {
    const int beg = seg_ptr[s], end = seg_ptr[s + 1];
    if (end <= beg) {
      if (col_ok) out[(size_t)s * d4 + lane] = zero4();
      continue;
    }
    const int cb = beg >> SEGSUM_PIECE_LOG2, ce = (end - 1) >> SEGSUM_PIECE_LOG2;
    if (cb == ce) continue;                                                // inside one piece: written by the walk
    float4 acc = zero4();
    if (col_ok) {
      acc = part[((size_t)cb * 2 + ((beg & (SEGSUM_PIECE - 1)) == 0 ? 0 : 1)) * d4 + lane];  // first piece: its last segment, unless it starts the piece
      int c = cb + 1;
      for (; c + 16 <= ce + 1; c += 16) {
        float4 q[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) q[u] = part[(size_t)(c + u) * 2 * d4 + lane];
#pragma unroll
        for (int u = 0; u < 16; ++u) acc = add4(acc, q[u]);
      }
      for (; c <= ce; ++c) acc = add4(acc, part[(size_t)c * 2 * d4 + lane]);
      out[(size_t)s * d4 + lane] = relu_of ? relu_gate4(relu_of[(size_t)s * d4 + lane], acc) : acc;
    }
  }
}

// rows per segment between the short-segment kernel's and the block-per-segment kernels' ranges: fixed pieces (robust to skew)
static bool segsum_pieces(int n_seg, long long n_rows, int d4) { return d4 <= 64 && n_rows > 2LL * n_seg && n_rows <= 32LL * n_seg && n_rows < (1LL << 31) - 64; }

static int segsum_splits(int n_seg, long long n_rows) {
  if (n_seg <= 0 || n_rows < 512LL * n_seg) return 1;
  int S = 2048 / n_seg;
  if (S > 64) S = 64;
  return S < 2 ? 1 : S;
}

size_t segment_sum_rows_workspace(int n_seg, long long n_rows, int d) {
  if (d / 4 > 64) return 0;                                  // wider than a wave of float4: a wave per segment, no workspace
  const int S = segsum_splits(n_seg, n_rows);
  if (S > 1) return (size_t)n_seg * S * d * sizeof(float);
  if (segsum_pieces(n_seg, n_rows, d / 4)) return (size_t)ceil_div(n_rows, (long long)SEGSUM_PIECE) * 2 * d * sizeof(float);
  return 0;
}

int segment_sum_rows(int n_seg, int d, const int32_t* seg_ptr, const int32_t* order, const float* src, const int32_t* row_mask, float* out,
                     hipStream_t st, long long n_rows_hint, void* ws, size_t ws_bytes, const float* relu_src) {
  const int d4 = d / 4;
  const float4* relu_of = (const float4*)relu_src;           // out = (relu_src > 0) ? sum : 0, element by element (nullable)
  const int S = segsum_splits(n_seg, n_rows_hint);
  if (S > 1 && d4 <= 64 && ws && ws_bytes >= segment_sum_rows_workspace(n_seg, n_rows_hint, d)) {
    TEMP_LAUNCH(K_SEGMENT_SUM, k_segment_sum_part, dim3(S, n_seg), dim3(256), 0, st, S, d4, seg_ptr, order, (const float4*)src, row_mask, (float4*)ws);
    TEMP_LAUNCH(K_SEGMENT_SUM, k_segment_sum_fin, dim3(ceil_div((long long)n_seg * d4, 256)), dim3(256), 0, st, n_seg, S, d4, (const float4*)ws, relu_of, (float4*)out);
    return launch_status();
  }
  if (S <= 1 && segsum_pieces(n_seg, n_rows_hint, d4) && ws && ws_bytes >= segment_sum_rows_workspace(n_seg, n_rows_hint, d)) {
    const int n_pieces = (int)ceil_div(n_rows_hint, (long long)SEGSUM_PIECE);
    TEMP_LAUNCH(K_SEGMENT_SUM, k_segment_sum_pieces, dim3(ceil_div(n_pieces, 4)), dim3(256), 0, st, n_seg, (int)n_rows_hint, d4, seg_ptr, order,
                (const float4*)src, row_mask, relu_of, (float4*)out, (float4*)ws);
    int grid = ceil_div(n_seg, 4);
    if (grid > 2048) grid = 2048;
    TEMP_LAUNCH(K_SEGMENT_SUM, k_segment_sum_pieces_fin, dim3(grid), dim3(256), 0, st, n_seg, d4, seg_ptr, (const float4*)ws, relu_of, (float4*)out);
    return launch_status();
  }
  if (n_rows_hint > 32LL * n_seg && d4 <= 64) {
    if (n_rows_hint >= 96LL * n_seg)
      TEMP_LAUNCH(K_SEGMENT_SUM, k_segment_sum_rows_blk<16>, dim3(n_seg < 4096 ? n_seg : 4096), dim3(16 * 64), 0, st, n_seg, d4, seg_ptr, order,
                  (const float4*)src, row_mask, relu_of, (float4*)out);
    else
      TEMP_LAUNCH(K_SEGMENT_SUM, k_segment_sum_rows_blk<4>, dim3(n_seg < 4096 ? n_seg : 4096), dim3(4 * 64), 0, st, n_seg, d4, seg_ptr, order,
                  (const float4*)src, row_mask, relu_of, (float4*)out);
    return launch_status();
  }
  const bool short_segs = n_rows_hint > 0 && n_rows_hint <= 2LL * n_seg;      // four segments per wave in lockstep
  int grid = ceil_div(n_seg, short_segs ? 16 : 4);
  if (grid > 2048) grid = 2048;
#define TEMP_SEGSUM(...)                                                                                                                     \
  do {                                                                                                                                      \
    if (short_segs) TEMP_LAUNCH(K_SEGMENT_SUM, (k_segment_sum_rows_short<__VA_ARGS__>), dim3(grid), dim3(256), 0, st, n_seg, d4, seg_ptr, order,      \
                                (const float4*)src, row_mask, relu_of, (float4*)out);                                                       \
    else TEMP_LAUNCH(K_SEGMENT_SUM, (k_segment_sum_rows<__VA_ARGS__>), dim3(grid), dim3(256), 0, st, n_seg, d4, seg_ptr, order, (const float4*)src,   \
                     row_mask, relu_of, (float4*)out);                                                                                      \
  } while (0)
  // d4 > 64: the lanes of the block, split and piece kernels are the columns of a row, so wider rows come here whatever the segment
  // lengths, and the wave walks its segment once per 64 columns
  if (d4 <= 8) TEMP_SEGSUM(8); else if (d4 <= 16) TEMP_SEGSUM(16); else if (d4 <= 32) TEMP_SEGSUM(32); else if (d4 <= 64) TEMP_SEGSUM(64);
  else TEMP_SEGSUM(64, true);
#undef TEMP_SEGSUM
  return launch_status();
}
// ---- the diachronic entity table (DE: ent * [1 | sin(t w + b)]) and its adjoint ------------------------------------------------
// out[(b N + j), c] = ent[j, c]                                            c <  ds = d / 2
//                   = ent[j, c] * sin(t_b * w[j, c - ds] + b[j, c - ds])   c >= ds
// One thread owns one entity and V columns (V = 4: float4 on every stream; V = 1 for the widths float4 does not divide) and walks
// the B timestamps: ent / w / b are read once, the adjoint sums its B terms in registers in ascending b and OVERWRITES d_ent /
// d_w / d_b -- no atomics, no workspace, no second launch.  Nothing is kept between the passes: the backward forms sin / cos anew.
template <int V> struct alignas(4 * V) DeVec { float v[V]; };

// The argument as torch forms it: t * w and + b are TWO rounded fp32 operations.  At t ~ 4e3 a fused multiply-add moves the
// argument by up to half an ulp of a number in the thousands, i.e. the sine by 1e-5 .. 1e-4.  Contraction is switched off for
// exactly these two operations (the build's default contracts a * b + c wherever it sees one).
__device__ __forceinline__ float de_arg(float t, float w, float b) {
#pragma clang fp contract(off)
  const float p = t * w;
  return p + b;
}

template <int V>
__global__ void __launch_bounds__(256) k_diachronic_fwd(int B, int N, int d, const float* __restrict__ ent, const float* __restrict__ w,
                                                        const float* __restrict__ bias, const float* __restrict__ t, float* __restrict__ out) {
  using Vec = DeVec<V>;
  const int dv = d / V, dsv = (d / 2) / V, dtv = dv - dsv;
  const size_t plane = (size_t)N * dv;                           // Vecs per timestamp
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= plane) return;
  const int j = (int)(i / dv), c = (int)(i - (size_t)j * dv);
  const Vec e = ((const Vec*)ent)[i];
  Vec* __restrict__ o = (Vec*)out;
  if (c < dsv) {                                                 // the static half is a copy
    for (int b = 0; b < B; ++b) o[(size_t)b * plane + i] = e;
    return;
  }
  const size_t k = (size_t)j * dtv + (c - dsv);
  const Vec wv = ((const Vec*)w)[k], bv = ((const Vec*)bias)[k];
  for (int b = 0; b < B; ++b) {
    const float tb = t[b];
    Vec r;
#pragma unroll
    for (int u = 0; u < V; ++u) r.v[u] = e.v[u] * sinf(de_arg(tb, wv.v[u], bv.v[u]));
    o[(size_t)b * plane + i] = r;
  }
}

template <int V>
__global__ void __launch_bounds__(256) k_diachronic_bwd(int B, int N, int d, const float* __restrict__ ent, const float* __restrict__ w,
                                                        const float* __restrict__ bias, const float* __restrict__ t,
                                                        const float* __restrict__ d_out, float* __restrict__ d_ent, float* __restrict__ d_w,
                                                        float* __restrict__ d_b) {
  using Vec = DeVec<V>;
  const int dv = d / V, dsv = (d / 2) / V, dtv = dv - dsv;
  const size_t plane = (size_t)N * dv;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= plane) return;
  const int j = (int)(i / dv), c = (int)(i - (size_t)j * dv);
  const Vec* __restrict__ g = (const Vec*)d_out;
  Vec ae;
#pragma unroll
  for (int u = 0; u < V; ++u) ae.v[u] = 0.f;
  if (c < dsv) {
#pragma unroll 4
    for (int b = 0; b < B; ++b) {
      const Vec gv = g[(size_t)b * plane + i];
#pragma unroll
      for (int u = 0; u < V; ++u) ae.v[u] += gv.v[u];
    }
    ((Vec*)d_ent)[i] = ae;
    return;
  }
  const size_t k = (size_t)j * dtv + (c - dsv);
  const Vec e = ((const Vec*)ent)[i], wv = ((const Vec*)w)[k], bv = ((const Vec*)bias)[k];
  Vec aw = ae, ab = ae;
#pragma unroll 4
  for (int b = 0; b < B; ++b) {
    const Vec gv = g[(size_t)b * plane + i];
    const float tb = t[b];
#pragma unroll
    for (int u = 0; u < V; ++u) {
      float sn, cs;
      sincosf(de_arg(tb, wv.v[u], bv.v[u]), &sn, &cs);
      const float gc = gv.v[u] * e.v[u] * cs;                    // d_out * ent * cos
      ae.v[u] += gv.v[u] * sn;
      ab.v[u] += gc;
      aw.v[u] += gc * tb;
    }
  }
  ((Vec*)d_ent)[i] = ae;
  ((Vec*)d_w)[k] = aw;
  ((Vec*)d_b)[k] = ab;
}

// float4 on every stream needs both halves of a row to start on a 16-byte boundary: d % 4 == 0 and (d / 2) % 4 == 0
static bool diachronic_vec(int d) { return d % 4 == 0 && (d / 2) % 4 == 0; }
static bool diachronic_args_ok(int B, int N, int d) {
  return B >= 1 && N >= 1 && d >= 2 && ((long long)N * d + 255) / 256 <= 0x7fffffffLL;       // (the grid: one thread per V columns)
}

// ---- the hyperplane projection of a table for B normals (HyTE: e - n_b (n_b . e), n_b = w_b / |w_b|) and its adjoint --------------
// One BLOCK of four waves owns one tile of HP_TILE_ROWS consecutive table rows (tile t = rows [32 t, 32 t + 32) whatever the grid:
// the blocks stride over the tiles), wave v its rows [8 v, 8 v + 8), and walks the B normals HP_CHUNK at a time.  LPR lanes share a
// row, one V-column vector each (d / V <= LPR), so a wave has G = 64 / LPR rows in flight and group g takes rows g, g + G, ... of the
// wave's eight; the row dots are xor butterflies over the LPR lanes (every lane of the group ends with the same bits).  (A wave per
// tile walked 32 / G rows one after the other: at N = 7 128 that is 223 waves on 256 CUs, each waiting out 16 - 32 load round
// trips.)  The chunk's normals live in registers: each wave forms them from w itself -- sum of squares by the same butterfly,
// n = w * (1 / sqrt) -- so there is no pre-kernel; LDS holds only the backward's four per-wave sums of a tile.
// Rows wider than 64 vectors take the *_wide kernels: one row per wave at a time, the lanes loop over the columns, and what the
// register kernels keep in registers (the normals, the running sums) is re-read from w / written through to its destination; there
// a wave owns a tile.
#define HP_TILE_ROWS TEMP_HYPERPLANE_TILE_ROWS
#define HP_CHUNK TEMP_HYPERPLANE_CHUNK                             // normals held on chip at a time

template <int LPR>
__device__ __forceinline__ float hp_group_sum(float v) {
#pragma unroll
  for (int m = 1; m < LPR; m <<= 1) v += __shfl_xor(v, m);
  return v;
}

// the chunk's normals [b0, b0 + HP_CHUNK) at this lane's columns (zero past B and past the row's width)
template <int V, int LPR>
__device__ __forceinline__ void hp_normals(int B, int dv, int b0, int col, bool col_ok, const DeVec<V>* __restrict__ w, DeVec<V> (&nrm)[HP_CHUNK]) {
#pragma unroll
  for (int k = 0; k < HP_CHUNK; ++k) {
    const int b = b0 + k;
    DeVec<V> wv;
#pragma unroll
    for (int u = 0; u < V; ++u) wv.v[u] = 0.f;
    if (col_ok && b < B) wv = w[(size_t)b * dv + col];
    float ss = 0.f;
#pragma unroll
    for (int u = 0; u < V; ++u) ss = fmaf(wv.v[u], wv.v[u], ss);
    ss = hp_group_sum<LPR>(ss);
    const float inv = b < B ? 1.0f / sqrtf(ss) : 0.f;
#pragma unroll
    for (int u = 0; u < V; ++u) nrm[k].v[u] = wv.v[u] * inv;
  }
}

template <int V, int LPR>
__global__ void __launch_bounds__(256) k_hyperplane_fwd(int B, int N, int d, const float* __restrict__ table, const float* __restrict__ w,
                                                        float* __restrict__ out) {
  using Vec = DeVec<V>;
  constexpr int G = 64 / LPR, WROWS = HP_TILE_ROWS / 4, RPG = WROWS / G;     // rows per wave, rows per group
  const int dv = d / V;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, grp = lane / LPR, col = lane - grp * LPR;
  const bool col_ok = col < dv;
  const int n_tiles = (int)(((long long)N + HP_TILE_ROWS - 1) / HP_TILE_ROWS);
  const size_t plane = (size_t)N * dv;
  Vec* __restrict__ o = (Vec*)out;
  for (int t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    for (int b0 = 0; b0 < B; b0 += HP_CHUNK) {
      Vec nrm[HP_CHUNK];
      hp_normals<V, LPR>(B, dv, b0, col, col_ok, (const Vec*)w, nrm);
      for (int j = 0; j < RPG; ++j) {
        const long long i = (long long)t * HP_TILE_ROWS + wv * WROWS + j * G + grp;
        const bool ok = col_ok && i < N;
        Vec e;
#pragma unroll
        for (int u = 0; u < V; ++u) e.v[u] = 0.f;
        if (ok) e = ((const Vec*)table)[(size_t)i * dv + col];
        float dot[HP_CHUNK];
#pragma unroll
        for (int k = 0; k < HP_CHUNK; ++k) {
          float a = 0.f;
#pragma unroll
          for (int u = 0; u < V; ++u) a = fmaf(nrm[k].v[u], e.v[u], a);
          dot[k] = a;
        }
#pragma unroll
        for (int k = 0; k < HP_CHUNK; ++k) dot[k] = hp_group_sum<LPR>(dot[k]);
#pragma unroll
        for (int k = 0; k < HP_CHUNK; ++k) {
          if (ok && b0 + k < B) {
            Vec r;
#pragma unroll
            for (int u = 0; u < V; ++u) r.v[u] = fmaf(-nrm[k].v[u], dot[k], e.v[u]);
            o[(size_t)(b0 + k) * plane + (size_t)i * dv + col] = r;
          }
        }
      }
    }
  }
}

// Adjoint, first launch.  Per row i and normal b: s = n_b . G_bi, p = n_b . e_i;  d_table[i] += G_bi - n_b s (ascending b: in
// registers within a chunk, through d_table itself -- the same lane re-reads what it wrote -- from one chunk to the next) and the
// tile's share of -d_n_b, sum_i p G_bi + s e_i: a group adds its rows in ascending order, the G groups of a wave meet in a butterfly,
// the four waves in LDS in wave order, and wave 0 writes part[t][b][:].  Every (t, b) is written exactly once, so the workspace
// needs no zero fill.
template <int V, int LPR>
__global__ void __launch_bounds__(256) k_hyperplane_bwd(int B, int N, int d, const float* __restrict__ table, const float* __restrict__ w,
                                                        const float* __restrict__ d_out, float* d_table, float* __restrict__ part) {
  using Vec = DeVec<V>;
  constexpr int G = 64 / LPR, WROWS = HP_TILE_ROWS / 4, RPG = WROWS / G;     // rows per wave, rows per group
  const int dv = d / V;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, grp = lane / LPR, col = lane - grp * LPR;
  const bool col_ok = col < dv;
  const int n_tiles = (int)(((long long)N + HP_TILE_ROWS - 1) / HP_TILE_ROWS);
  const size_t plane = (size_t)N * dv;
  const Vec* __restrict__ gp = (const Vec*)d_out;
  Vec* dt = (Vec*)d_table;
  __shared__ Vec red[4][HP_CHUNK][LPR];                                     // the four waves' sums of the chunk: 32 KB at V = 4, LPR = 64
  for (int t = blockIdx.x; t < n_tiles; t += gridDim.x) {                 // (block-uniform: the barriers below are reached by all)
    for (int b0 = 0; b0 < B; b0 += HP_CHUNK) {
      Vec nrm[HP_CHUNK], acc[HP_CHUNK];
      hp_normals<V, LPR>(B, dv, b0, col, col_ok, (const Vec*)w, nrm);
#pragma unroll
      for (int k = 0; k < HP_CHUNK; ++k)
#pragma unroll
        for (int u = 0; u < V; ++u) acc[k].v[u] = 0.f;
#pragma unroll 1
      for (int j = 0; j < RPG; ++j) {
        const long long i = (long long)t * HP_TILE_ROWS + wv * WROWS + j * G + grp;
        const bool ok = col_ok && i < N;
        const size_t at_i = (size_t)i * dv + col;
        Vec e, at, g[HP_CHUNK];
#pragma unroll
        for (int u = 0; u < V; ++u) e.v[u] = at.v[u] = 0.f;
        if (ok) e = ((const Vec*)table)[at_i];
        if (ok && b0 > 0) at = dt[at_i];
#pragma unroll
        for (int k = 0; k < HP_CHUNK; ++k) {
#pragma unroll
          for (int u = 0; u < V; ++u) g[k].v[u] = 0.f;
          if (ok && b0 + k < B) g[k] = gp[(size_t)(b0 + k) * plane + at_i];
        }
        float s[HP_CHUNK], p[HP_CHUNK];
#pragma unroll
        for (int k = 0; k < HP_CHUNK; ++k) {
          float a = 0.f, c = 0.f;
#pragma unroll
          for (int u = 0; u < V; ++u) { a = fmaf(nrm[k].v[u], g[k].v[u], a); c = fmaf(nrm[k].v[u], e.v[u], c); }
          s[k] = a; p[k] = c;
        }
#pragma unroll
        for (int k = 0; k < HP_CHUNK; ++k) { s[k] = hp_group_sum<LPR>(s[k]); p[k] = hp_group_sum<LPR>(p[k]); }
#pragma unroll
        for (int k = 0; k < HP_CHUNK; ++k) {
#pragma unroll
          for (int u = 0; u < V; ++u) {
            at.v[u] += fmaf(-nrm[k].v[u], s[k], g[k].v[u]);
            acc[k].v[u] += fmaf(p[k], g[k].v[u], s[k] * e.v[u]);
          }
        }
        if (ok) dt[at_i] = at;
      }
#pragma unroll
      for (int k = 0; k < HP_CHUNK; ++k) {
#pragma unroll
        for (int u = 0; u < V; ++u)
#pragma unroll
          for (int m = LPR; m < 64; m <<= 1) acc[k].v[u] += __shfl_xor(acc[k].v[u], m);
        if (grp == 0) red[wv][k][col] = acc[k];
      }
      __syncthreads();
      if (wv == 0 && grp == 0 && col_ok) {
#pragma unroll
        for (int k = 0; k < HP_CHUNK; ++k) {
          if (b0 + k < B) {
            Vec r;
#pragma unroll
            for (int u = 0; u < V; ++u) r.v[u] = ((red[0][k][col].v[u] + red[1][k][col].v[u]) + red[2][k][col].v[u]) + red[3][k][col].v[u];
            ((Vec*)part)[((size_t)t * B + (b0 + k)) * dv + col] = r;
          }
        }
      }
      __syncthreads();                                                     // red is rewritten by the next chunk / tile
    }
  }
}

template <int V>
__global__ void __launch_bounds__(256) k_hyperplane_fwd_wide(int B, int N, int d, const float* __restrict__ table, const float* __restrict__ w,
                                                             float* __restrict__ out) {
  using Vec = DeVec<V>;
  const int dv = d / V;
  const int lane = threadIdx.x & 63;
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = (gridDim.x * blockDim.x) >> 6;
  const int n_tiles = (int)(((long long)N + HP_TILE_ROWS - 1) / HP_TILE_ROWS);
  const size_t plane = (size_t)N * dv;
  const Vec* __restrict__ wp = (const Vec*)w;
  const Vec* __restrict__ tp = (const Vec*)table;
  Vec* __restrict__ o = (Vec*)out;
  for (int t = wave; t < n_tiles; t += nwaves) {
    for (int b0 = 0; b0 < B; b0 += HP_CHUNK) {
      const int nb = min(HP_CHUNK, B - b0);
      float inv[HP_CHUNK];
#pragma unroll
      for (int k = 0; k < HP_CHUNK; ++k) {
        float ss = 0.f;
        if (k < nb)
          for (int c = lane; c < dv; c += 64) {
            const Vec wv = wp[(size_t)(b0 + k) * dv + c];
#pragma unroll
            for (int u = 0; u < V; ++u) ss = fmaf(wv.v[u], wv.v[u], ss);
          }
        ss = hp_group_sum<64>(ss);
        inv[k] = k < nb ? 1.0f / sqrtf(ss) : 0.f;
      }
      for (int r = 0; r < HP_TILE_ROWS; ++r) {
        const long long i = (long long)t * HP_TILE_ROWS + r;
        if (i >= N) break;                                           // (wave-uniform)
        float dot[HP_CHUNK];
#pragma unroll
        for (int k = 0; k < HP_CHUNK; ++k) dot[k] = 0.f;
        for (int c = lane; c < dv; c += 64) {
          const Vec e = tp[(size_t)i * dv + c];
#pragma unroll
          for (int k = 0; k < HP_CHUNK; ++k)
            if (k < nb) {
              const Vec wv = wp[(size_t)(b0 + k) * dv + c];
#pragma unroll
              for (int u = 0; u < V; ++u) dot[k] = fmaf(wv.v[u] * inv[k], e.v[u], dot[k]);
            }
        }
#pragma unroll
        for (int k = 0; k < HP_CHUNK; ++k) dot[k] = hp_group_sum<64>(dot[k]);
        for (int c = lane; c < dv; c += 64) {
          const Vec e = tp[(size_t)i * dv + c];
#pragma unroll
          for (int k = 0; k < HP_CHUNK; ++k)
            if (k < nb) {
              const Vec wv = wp[(size_t)(b0 + k) * dv + c];
              Vec q;
#pragma unroll
              for (int u = 0; u < V; ++u) q.v[u] = fmaf(-(wv.v[u] * inv[k]), dot[k], e.v[u]);
              o[(size_t)(b0 + k) * plane + (size_t)i * dv + c] = q;
            }
        }
      }
    }
  }
}

// (the running sums go through their destinations: part[t][b][c] is overwritten by the tile's first row and added to by the same
// lane for the later ones, d_table[i][c] by the first chunk and the later ones -- the order of the additions is that of the
// register kernels: rows ascending, b ascending)
template <int V>
__global__ void __launch_bounds__(256) k_hyperplane_bwd_wide(int B, int N, int d, const float* __restrict__ table, const float* __restrict__ w,
                                                             const float* __restrict__ d_out, float* d_table, float* part) {
  using Vec = DeVec<V>;
  const int dv = d / V;
  const int lane = threadIdx.x & 63;
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = (gridDim.x * blockDim.x) >> 6;
  const int n_tiles = (int)(((long long)N + HP_TILE_ROWS - 1) / HP_TILE_ROWS);
  const size_t plane = (size_t)N * dv;
  const Vec* __restrict__ wp = (const Vec*)w;
  const Vec* __restrict__ tp = (const Vec*)table;
  const Vec* __restrict__ gp = (const Vec*)d_out;
  Vec* dt = (Vec*)d_table;
  Vec* pp = (Vec*)part;
  for (int t = wave; t < n_tiles; t += nwaves) {
    for (int b0 = 0; b0 < B; b0 += HP_CHUNK) {
      const int nb = min(HP_CHUNK, B - b0);
      float inv[HP_CHUNK];
#pragma unroll
      for (int k = 0; k < HP_CHUNK; ++k) {
        float ss = 0.f;
        if (k < nb)
          for (int c = lane; c < dv; c += 64) {
            const Vec wv = wp[(size_t)(b0 + k) * dv + c];
#pragma unroll
            for (int u = 0; u < V; ++u) ss = fmaf(wv.v[u], wv.v[u], ss);
          }
        ss = hp_group_sum<64>(ss);
        inv[k] = k < nb ? 1.0f / sqrtf(ss) : 0.f;
      }
      for (int r = 0; r < HP_TILE_ROWS; ++r) {
        const long long i = (long long)t * HP_TILE_ROWS + r;
        if (i >= N) break;                                           // (wave-uniform)
        float s[HP_CHUNK], p[HP_CHUNK];
#pragma unroll
        for (int k = 0; k < HP_CHUNK; ++k) s[k] = p[k] = 0.f;
        for (int c = lane; c < dv; c += 64) {
          const Vec e = tp[(size_t)i * dv + c];
#pragma unroll
          for (int k = 0; k < HP_CHUNK; ++k)
            if (k < nb) {
              const Vec wv = wp[(size_t)(b0 + k) * dv + c];
              const Vec g = gp[(size_t)(b0 + k) * plane + (size_t)i * dv + c];
#pragma unroll
              for (int u = 0; u < V; ++u) {
                const float n = wv.v[u] * inv[k];
                s[k] = fmaf(n, g.v[u], s[k]);
                p[k] = fmaf(n, e.v[u], p[k]);
              }
            }
        }
#pragma unroll
        for (int k = 0; k < HP_CHUNK; ++k) { s[k] = hp_group_sum<64>(s[k]); p[k] = hp_group_sum<64>(p[k]); }
        for (int c = lane; c < dv; c += 64) {
          const size_t at_i = (size_t)i * dv + c;
          const Vec e = tp[at_i];
          Vec at;
#pragma unroll
          for (int u = 0; u < V; ++u) at.v[u] = 0.f;
          if (b0 > 0) at = dt[at_i];
#pragma unroll
          for (int k = 0; k < HP_CHUNK; ++k)
            if (k < nb) {
              const Vec wv = wp[(size_t)(b0 + k) * dv + c];
              const Vec g = gp[(size_t)(b0 + k) * plane + at_i];
              const size_t at_p = ((size_t)t * B + (b0 + k)) * dv + c;
              Vec a;
#pragma unroll
              for (int u = 0; u < V; ++u) a.v[u] = 0.f;
              if (r > 0) a = pp[at_p];
#pragma unroll
              for (int u = 0; u < V; ++u) {
                const float n = wv.v[u] * inv[k];
                at.v[u] += fmaf(-n, s[k], g.v[u]);
                a.v[u] += fmaf(p[k], g.v[u], s[k] * e.v[u]);
              }
              pp[at_p] = a;
            }
          dt[at_i] = at;
        }
      }
    }
  }
}

// Adjoint, second launch: block b adds the tiles' partials of -d_n_b in ascending tile order (one column per thread, 32 loads in
// flight, the additions in order), parks the sums in d_w while the block forms |w_b|^2 and w_b . sum (wave butterflies, then the
// four waves in wave order), and applies the Jacobian of w -> w / |w|:  d_w_b = (d_n_b - n_b (n_b . d_n_b)) / |w_b|.
__global__ void __launch_bounds__(256) k_hyperplane_bwd_finish(int B, int n_tiles, int d, const float* __restrict__ w, const float* __restrict__ part,
                                                               float* d_w) {
  __shared__ float red[2][4];
  const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t stride = (size_t)B * d;
  float ss = 0.f, wa = 0.f;
  for (int c = threadIdx.x; c < d; c += 256) {
    const float* __restrict__ p = part + (size_t)b * d + c;
    float acc = 0.f;
    int t = 0;
    for (; t + 32 <= n_tiles; t += 32) {
      float q[32];
#pragma unroll
      for (int u = 0; u < 32; ++u) q[u] = p[(size_t)(t + u) * stride];
#pragma unroll
      for (int u = 0; u < 32; ++u) acc += q[u];
    }
    for (; t < n_tiles; ++t) acc += p[(size_t)t * stride];
    const float wv = w[(size_t)b * d + c];
    d_w[(size_t)b * d + c] = acc;
    ss = fmaf(wv, wv, ss);
    wa = fmaf(wv, acc, wa);
  }
  ss = hp_group_sum<64>(ss);
  wa = hp_group_sum<64>(wa);
  if (lane == 0) { red[0][wave] = ss; red[1][wave] = wa; }
  __syncthreads();
  ss = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
  wa = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
  const float inv = 1.0f / sqrtf(ss);
  const float na = wa * inv;                                          // n_b . acc  (acc = -d_n_b)
  for (int c = threadIdx.x; c < d; c += 256) {
    const float n = w[(size_t)b * d + c] * inv;
    const float acc = d_w[(size_t)b * d + c];                          // (this thread's own store)
    d_w[(size_t)b * d + c] = fmaf(n, na, -acc) * inv;
  }
}

static bool hyperplane_args_ok(int B, int N, int d) { return B >= 1 && N >= 1 && d >= 1; }
static int hyperplane_tiles(int N) { return (int)(((long long)N + HP_TILE_ROWS - 1) / HP_TILE_ROWS); }
static int hyperplane_grid(int N, bool wide) {                      // a block per tile; a wave per tile in the column-loop kernels
  const int g = wide ? ceil_div(hyperplane_tiles(N), 4) : hyperplane_tiles(N);
  return g > 8192 ? 8192 : g;
}
// kernel<V, LPR> for rows of up to 16 / 32 / 64 vectors, kernel_wide<V> beyond; V = 4 when float4 divides the row
#define TEMP_HYPERPLANE(KID, kern, ...)                                                                                                  \
  do {                                                                                                                                   \
    const int dv = d % 4 == 0 ? d / 4 : d;                                                                                               \
    const dim3 grid(hyperplane_grid(N, dv > 64)), block(256);                                                                            \
    if (d % 4 == 0) {                                                                                                                    \
      if (dv <= 16) TEMP_LAUNCH(KID, (kern<4, 16>), grid, block, 0, st, __VA_ARGS__);                                                    \
      else if (dv <= 32) TEMP_LAUNCH(KID, (kern<4, 32>), grid, block, 0, st, __VA_ARGS__);                                               \
      else if (dv <= 64) TEMP_LAUNCH(KID, (kern<4, 64>), grid, block, 0, st, __VA_ARGS__);                                               \
      else TEMP_LAUNCH(KID, (kern##_wide<4>), grid, block, 0, st, __VA_ARGS__);                                                          \
    } else {                                                                                                                             \
      if (dv <= 16) TEMP_LAUNCH(KID, (kern<1, 16>), grid, block, 0, st, __VA_ARGS__);                                                    \
      else if (dv <= 32) TEMP_LAUNCH(KID, (kern<1, 32>), grid, block, 0, st, __VA_ARGS__);                                               \
      else if (dv <= 64) TEMP_LAUNCH(KID, (kern<1, 64>), grid, block, 0, st, __VA_ARGS__);                                               \
      else TEMP_LAUNCH(KID, (kern##_wide<1>), grid, block, 0, st, __VA_ARGS__);                                                          \
    }                                                                                                                                    \
  } while (0)

// ---- the pair table of two tables for B windows (SimplE: [a | a_inv]) and its adjoint ------------------------------------------
// out[(b N + i), :] = [a[i, :] | a_inv[i, :]], rows of width 2 d.  As in the diachronic pass one thread owns one row and V columns of
// BOTH halves (V = 4: float4 on every stream -- d % 4 == 0 puts both halves of an output row on 16-byte boundaries; V = 1 otherwise)
// and walks the B windows: a / a_inv are read once; the adjoint adds its B terms in registers in ascending b and OVERWRITES d_a /
// d_a_inv -- no atomics, no workspace, no second launch.
template <int V>
__global__ void __launch_bounds__(256) k_pair_rows_fwd(int B, int N, int d, const float* __restrict__ a, const float* __restrict__ a_inv,
                                                       float* __restrict__ out) {
  using Vec = DeVec<V>;
  const int dv = d / V;
  const size_t plane = (size_t)N * dv;                           // Vecs per table
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= plane) return;
  const size_t j = i / dv, c = i - j * dv;
  const Vec x = ((const Vec*)a)[i], y = ((const Vec*)a_inv)[i];
  Vec* __restrict__ o = (Vec*)out + j * 2 * dv + c;
  for (int b = 0; b < B; ++b) {
    o[(size_t)b * 2 * plane] = x;
    o[(size_t)b * 2 * plane + dv] = y;
  }
}

template <int V>
__global__ void __launch_bounds__(256) k_pair_rows_bwd(int B, int N, int d, const float* __restrict__ d_out, float* __restrict__ d_a,
                                                       float* __restrict__ d_a_inv) {
  using Vec = DeVec<V>;
  const int dv = d / V;
  const size_t plane = (size_t)N * dv;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= plane) return;
  const size_t j = i / dv, c = i - j * dv;
  const Vec* __restrict__ g = (const Vec*)d_out + j * 2 * dv + c;
  Vec sx, sy;
#pragma unroll
  for (int u = 0; u < V; ++u) sx.v[u] = sy.v[u] = 0.f;
#pragma unroll 4
  for (int b = 0; b < B; ++b) {
    const Vec gx = g[(size_t)b * 2 * plane], gy = g[(size_t)b * 2 * plane + dv];
#pragma unroll
    for (int u = 0; u < V; ++u) { sx.v[u] += gx.v[u]; sy.v[u] += gy.v[u]; }
  }
  ((Vec*)d_a)[i] = sx;
  ((Vec*)d_a_inv)[i] = sy;
}

static bool pair_rows_args_ok(int B, int N, int d) {
  return B >= 1 && N >= 1 && d >= 1 && ((long long)N * d + 255) / 256 <= 0x7fffffffLL;        // (the grid: one thread per V columns)
}
}  // namespace temp

using namespace temp;

extern "C" {

int temp_gather_rows(int n, int d, const float* table, const int32_t* idx, float* out, void* stream) {
  if (n < 0 || d <= 0 || (n > 0 && (!table || !idx || !out))) return TEMP_E_BADARG;
  if (d % 4) return TEMP_E_UNSUPPORTED;
  if (n == 0) return TEMP_OK;
  int grid = ceil_div((long long)n * (d / 4), 256);
  if (grid > 4096) grid = 4096;
  TEMP_LAUNCH(K_GATHER_ROWS, k_gather_rows, dim3(grid), dim3(256), 0, (hipStream_t)stream, n, d / 4, (const float4*)table, idx, (float4*)out);
  return launch_status();
}

int temp_scatter_add_rows(int n, int d, const float* src, const int32_t* idx, float* table, void* stream) {
  if (n < 0 || d <= 0 || (n > 0 && (!table || !idx || !src))) return TEMP_E_BADARG;
  if (n == 0) return TEMP_OK;
  int grid = ceil_div((long long)n * d, 256);
  if (grid > 4096) grid = 4096;
  TEMP_LAUNCH(K_SCATTER_ADD, k_scatter_add_rows, dim3(grid), dim3(256), 0, (hipStream_t)stream, n, d, src, idx, table);
  return launch_status();
}

size_t temp_segment_sum_rows_workspace(int n_seg, int n_rows, int d) { return (n_seg <= 0 || d <= 0) ? 0 : segment_sum_rows_workspace(n_seg, n_rows, d); }

int temp_segment_sum_rows(int n_seg, int n_rows, int d, const int32_t* seg_ptr, const int32_t* order, const float* src, float* out,
                          void* workspace, size_t workspace_bytes, void* stream) {
  if (n_seg < 0 || d <= 0 || (n_seg > 0 && (!seg_ptr || !src || !out))) return TEMP_E_BADARG;
  if (d % 4) return TEMP_E_UNSUPPORTED;
  return segment_sum_rows(n_seg, d, seg_ptr, order, src, nullptr, out, (hipStream_t)stream, n_rows, workspace, workspace_bytes);
}

int temp_segment_sum_rows_relu(int n_seg, int n_rows, int d, const int32_t* seg_ptr, const int32_t* order, const float* src, const float* relu_of,
                               float* out, void* workspace, size_t workspace_bytes, void* stream) {
  if (n_seg < 0 || d <= 0 || (n_seg > 0 && (!seg_ptr || !src || !out || !relu_of))) return TEMP_E_BADARG;
  if (d % 4) return TEMP_E_UNSUPPORTED;
  return segment_sum_rows(n_seg, d, seg_ptr, order, src, nullptr, out, (hipStream_t)stream, n_rows, workspace, workspace_bytes, relu_of);
}

int temp_gather_rows_keys(int n, int d, const float* table, const int32_t* idx, float* out, uint32_t* row_keys, uint32_t* col_keys, void* stream) {
  if (n < 0 || d <= 0 || (n > 0 && (!table || !idx || !out))) return TEMP_E_BADARG;
  if (d % 4 || d > 256) return TEMP_E_UNSUPPORTED;
  if (n == 0) return TEMP_OK;
  launch_gather_rows_keys(n, d, table, idx, out, row_keys, col_keys, col_keys ? col_keys + d : nullptr, (hipStream_t)stream);
  return launch_status();
}

int temp_diachronic_rows_fwd(int B, int N, int d, const float* ent, const float* w, const float* b, const float* t, float* out, void* stream) {
  if (!diachronic_args_ok(B, N, d) || !ent || !w || !b || !t || !out) return TEMP_E_BADARG;
  if (diachronic_vec(d))
    TEMP_LAUNCH(K_DIACHRONIC_FWD, k_diachronic_fwd<4>, dim3(ceil_div((long long)N * (d / 4), 256)), dim3(256), 0, (hipStream_t)stream, B, N, d, ent, w, b, t, out);
  else
    TEMP_LAUNCH(K_DIACHRONIC_FWD, k_diachronic_fwd<1>, dim3(ceil_div((long long)N * d, 256)), dim3(256), 0, (hipStream_t)stream, B, N, d, ent, w, b, t, out);
  return launch_status();
}

int temp_diachronic_rows_bwd(int B, int N, int d, const float* ent, const float* w, const float* b, const float* t, const float* d_out, float* d_ent,
                             float* d_w, float* d_b, void* stream) {
  if (!diachronic_args_ok(B, N, d) || !ent || !w || !b || !t || !d_out || !d_ent || !d_w || !d_b) return TEMP_E_BADARG;
  if (diachronic_vec(d))
    TEMP_LAUNCH(K_DIACHRONIC_BWD, k_diachronic_bwd<4>, dim3(ceil_div((long long)N * (d / 4), 256)), dim3(256), 0, (hipStream_t)stream, B, N, d, ent, w, b, t,
                d_out, d_ent, d_w, d_b);
  else
    TEMP_LAUNCH(K_DIACHRONIC_BWD, k_diachronic_bwd<1>, dim3(ceil_div((long long)N * d, 256)), dim3(256), 0, (hipStream_t)stream, B, N, d, ent, w, b, t,
                d_out, d_ent, d_w, d_b);
  return launch_status();
}

size_t temp_hyperplane_rows_bwd_workspace(int B, int N, int d) {
  return hyperplane_args_ok(B, N, d) ? (size_t)hyperplane_tiles(N) * (size_t)B * (size_t)d * sizeof(float) : 0;
}

int temp_hyperplane_rows_fwd(int B, int N, int d, const float* table, const float* w, float* out, void* stream) {
  if (!hyperplane_args_ok(B, N, d) || !table || !w || !out) return TEMP_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  TEMP_HYPERPLANE(K_HYPERPLANE_FWD, k_hyperplane_fwd, B, N, d, table, w, out);
  return launch_status();
}

int temp_hyperplane_rows_bwd(int B, int N, int d, const float* table, const float* w, const float* d_out, float* d_table, float* d_w,
                             void* workspace, size_t workspace_bytes, void* stream) {
  if (!hyperplane_args_ok(B, N, d) || !table || !w || !d_out || !d_table || !d_w || !workspace) return TEMP_E_BADARG;
  if (workspace_bytes < temp_hyperplane_rows_bwd_workspace(B, N, d)) return TEMP_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  float* part = (float*)workspace;
  TEMP_HYPERPLANE(K_HYPERPLANE_BWD, k_hyperplane_bwd, B, N, d, table, w, d_out, d_table, part);
  TEMP_LAUNCH(K_HYPERPLANE_BWD_FINISH, k_hyperplane_bwd_finish, dim3(B), dim3(256), 0, st, B, hyperplane_tiles(N), d, w, (const float*)part, d_w);
  return launch_status();
}

int temp_pair_rows_fwd(int B, int N, int d, const float* a, const float* a_inv, float* out, void* stream) {
  if (!pair_rows_args_ok(B, N, d) || !a || !a_inv || !out) return TEMP_E_BADARG;
  if (d % 4 == 0)
    TEMP_LAUNCH(K_PAIR_ROWS_FWD, k_pair_rows_fwd<4>, dim3(ceil_div((long long)N * (d / 4), 256)), dim3(256), 0, (hipStream_t)stream, B, N, d, a, a_inv, out);
  else
    TEMP_LAUNCH(K_PAIR_ROWS_FWD, k_pair_rows_fwd<1>, dim3(ceil_div((long long)N * d, 256)), dim3(256), 0, (hipStream_t)stream, B, N, d, a, a_inv, out);
  return launch_status();
}

int temp_pair_rows_bwd(int B, int N, int d, const float* d_out, float* d_a, float* d_a_inv, void* stream) {
  if (!pair_rows_args_ok(B, N, d) || !d_out || !d_a || !d_a_inv) return TEMP_E_BADARG;
  if (d % 4 == 0)
    TEMP_LAUNCH(K_PAIR_ROWS_BWD, k_pair_rows_bwd<4>, dim3(ceil_div((long long)N * (d / 4), 256)), dim3(256), 0, (hipStream_t)stream, B, N, d, d_out, d_a, d_a_inv);
  else
    TEMP_LAUNCH(K_PAIR_ROWS_BWD, k_pair_rows_bwd<1>, dim3(ceil_div((long long)N * d, 256)), dim3(256), 0, (hipStream_t)stream, B, N, d, d_out, d_a, d_a_inv);
  return launch_status();
}

}  // extern "C"
