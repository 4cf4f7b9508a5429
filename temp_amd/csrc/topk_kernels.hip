// Filtered top-k selection over score rows (include/temp_amd.h: temp_filtered_topk): the answer list of a link-prediction query.
//
// One 256-thread workgroup per query row.  The row's current best k entries live in LDS, sorted under the total order
//   a before b  <=>  a.score > b.score  or  (a.score == b.score and a.id < b.id)
// (ids are unique, so no two real entries compare equal; an empty slot is (-inf, -1) and comes after every real entry, whose
// score is > -inf by the admissibility rule).  The row is streamed once, TOPK_CHUNK columns at a time with float4 loads; a lane
// compares each of its scores with the k-th entry and only the SURVIVORS are appended to an LDS buffer (one integer LDS add per
// lane that has any).  A chunk without survivors costs its loads, sixteen compares per lane and one barrier.  A chunk with
// survivors then
//   1. looks each survivor up in the row's filter list (binary search over global ids; the row's `keep` id passes) and blanks
//      the filtered ones -- the filter is paid per survivor, not per column;
//   2. with more than TOPK_PRUNE_MIN survivors (the first chunk of a fresh list, where everything beats -inf: an evaluation-sized
//      row is two chunks, so this chunk is most of its time) first drops what cannot matter: every lane takes the best of the
//      <= 16 survivors it owns, T = the k-th best of those 256 bests (ranked by counting), and a survivor that comes after T has
//      at least k survivors of its own chunk before it.  What remains lies in the columns of at most k lanes: <= 16 k entries;
//   3. sorts the buffer (bitonic, padded with empty slots to a power of two);
//   4. merges the two sorted sequences by rank: an element's new position is its own index plus the number of elements of the
//      OTHER sequence that come before it (one binary search each); positions < k are written to the second list buffer.
// Every slot of the new list is written exactly once because the merged positions are a permutation (unique keys; the empty list
// slots keep their relative order by index).  After the first few thousand columns the survivor rate is about k / columns seen,
// so the pass is bound by reading P * N * 4 bytes; the first chunk (everything beats -inf) and an ascending row (everything
// survives, chunk after chunk) pay step 2 and a sort of what it leaves, and are merely correct.
//
// The selection depends on the total order alone: the order in which survivors land in the buffer (the LDS counter) does not
// reach the result, so the output is bit-repeatable, and a list carried over from other column panels merges to the same list in
// any panel order.
//
// The MIXED instantiation (temp_filtered_topk_mix) selects over m = mix1(w[p], a, b) of two score rows -- the two-table post models'
// gated score -- without the mixed matrix ever existing: both rows are streamed with the same loads and the same one-chunk
// prefetch, and where the prefetched registers become the current chunk's values they are folded into ONE value per column,
// -inf when either operand is -inf (tested on the raw operands: w in {0, 1} would otherwise turn a -inf into 0 * inf = NaN or
// into a finite score), else mix1.  From there on the kernel is the plain one: a folded -inf fails the admissibility compare like
// a plain -inf.  The extra live state is the second prefetch set.
#include "common.hpp"
#include "mix.hpp"

namespace temp {
namespace {

constexpr int TOPK_THREADS = 256;
constexpr int TOPK_VEC = 4;                                        // float4 loads in flight per lane and chunk
constexpr int TOPK_CHUNK = TOPK_THREADS * 4 * TOPK_VEC;            // 4096 columns
constexpr int TOPK_OWN = TOPK_CHUNK / TOPK_THREADS;                // survivors a lane owns in the pruning step (slots tid + 256 i)
constexpr int TOPK_PRUNE_MIN = 1024;                               // below: the sort is cheaper than finding T
// dynamic LDS carve (every offset a multiple of 16): survivor scores / ids, the two list buffers (scores, ids), the two counters
// and the pruning threshold T (score bits, id)
constexpr int TOPK_OFF_CI = TOPK_CHUNK * 4;
constexpr int TOPK_OFF_LV = TOPK_CHUNK * 8;
constexpr int TOPK_OFF_LI = TOPK_OFF_LV + 2 * TEMP_TOPK_MAX * 4;
constexpr int TOPK_OFF_CNT = TOPK_OFF_LI + 2 * TEMP_TOPK_MAX * 4;
constexpr int TOPK_LDS = TOPK_OFF_CNT + 16;

__device__ __forceinline__ bool topk_before(float av, int ai, float bv, int bi) { return (av > bv) | ((av == bv) & (ai < bi)); }

// number of leading entries of the sorted sequence (v, id)[0, n) that come before (xv, xi)
__device__ __forceinline__ int topk_count_before(const float* v, const int* id, int n, float xv, int xi) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (topk_before(v[mid], id[mid], xv, xi)) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ float4 topk_load(const float* srow, int j, int N) {
  const float ninf = -__builtin_inff();
  return j < N ? ld4_nt(srow + j) : make_float4(ninf, ninf, ninf, ninf);
}

// one column of the mixed row: inadmissible (-inf) when either raw operand is
__device__ __forceinline__ float topk_fold1(float w, float a, float b) {
  const float ninf = -__builtin_inff();
  return ((a > ninf) & (b > ninf)) ? mix1(w, a, b) : ninf;
}
__device__ __forceinline__ float4 topk_fold(float w, float4 a, float4 b) {
  return make_float4(topk_fold1(w, a.x, b.x), topk_fold1(w, a.y, b.y), topk_fold1(w, a.z, b.z), topk_fold1(w, a.w, b.w));
}

// MIX = false: rows of `scores`; scores_b and w are not read (they come last, so every other argument keeps its kernarg offset and
// the plain instantiation compiles to the instructions it had before the template).  MIX = true: rows of mix1(w[p], scores, scores_b).
template <bool MIX>
__global__ void __launch_bounds__(TOPK_THREADS) k_filtered_topk(int N, int ld, int k, int col0, const float* __restrict__ scores,
                                                                const int32_t* __restrict__ filt_ptr, const int32_t* __restrict__ filt_ids,
                                                                const int32_t* __restrict__ keep, int carry, float* __restrict__ top_val,
                                                                int32_t* __restrict__ top_idx, const float* __restrict__ scores_b,
                                                                const float* __restrict__ w) {
  extern __shared__ __attribute__((aligned(16))) char topk_smem[];
  float* cv = reinterpret_cast<float*>(topk_smem);
  int* ci = reinterpret_cast<int*>(topk_smem + TOPK_OFF_CI);
  float* lv = reinterpret_cast<float*>(topk_smem + TOPK_OFF_LV);
  int* li = reinterpret_cast<int*>(topk_smem + TOPK_OFF_LI);
  int* cnt = reinterpret_cast<int*>(topk_smem + TOPK_OFF_CNT);
  const float ninf = -__builtin_inff();
  const int p = blockIdx.x, tid = threadIdx.x;
  const float* srow = scores + (size_t)p * ld;
  const float* brow = MIX ? scores_b + (size_t)p * ld : nullptr;
  const float wp = MIX ? w[p] : 0.f;
  const size_t out = (size_t)p * k;

  if (tid < k) {
    lv[tid] = carry ? top_val[out + tid] : ninf;
    li[tid] = carry ? top_idx[out + tid] : -1;
  }
  if (tid < 2) cnt[tid] = 0;
  const int f_lo = filt_ptr ? filt_ptr[p] : 0, f_hi = filt_ptr ? filt_ptr[p + 1] : 0;
  const int kp = keep ? keep[p] : -1;
  __syncthreads();

  int cur = 0;                                                     // which list buffer is current (wave-uniform)
  float thr_v = lv[k - 1];
  int thr_i = li[k - 1];
  float4 nx[TOPK_VEC], nb[MIX ? TOPK_VEC : 1];
#pragma unroll
  for (int u = 0; u < TOPK_VEC; ++u) {
    nx[u] = topk_load(srow, (u * TOPK_THREADS + tid) * 4, N);
    if constexpr (MIX) nb[u] = topk_load(brow, (u * TOPK_THREADS + tid) * 4, N);
  }

  int it = 0;
  for (int base = 0; base < N; base += TOPK_CHUNK, ++it) {
    float4 x[TOPK_VEC];
#pragma unroll
    for (int u = 0; u < TOPK_VEC; ++u) {
      if constexpr (MIX) x[u] = topk_fold(wp, nx[u], nb[u]); else x[u] = nx[u];
    }
    if (base + TOPK_CHUNK < N) {                                   // the next chunk's loads fly over this chunk's compares and barrier
#pragma unroll
      for (int u = 0; u < TOPK_VEC; ++u) {
        nx[u] = topk_load(srow, base + TOPK_CHUNK + (u * TOPK_THREADS + tid) * 4, N);
        if constexpr (MIX) nb[u] = topk_load(brow, base + TOPK_CHUNK + (u * TOPK_THREADS + tid) * 4, N);
      }
    }
    // two counters, by chunk parity: a fast wave that appends for chunk it + 1 cannot disturb the count a slow wave still has to
    // read for chunk it (it cannot pass the barrier of chunk it + 1 without that wave)
    int* c = cnt + (it & 1);
    unsigned m = 0;
#pragma unroll
    for (int u = 0; u < TOPK_VEC; ++u) {
      const int j = base + (u * TOPK_THREADS + tid) * 4;
      const float e[4] = {x[u].x, x[u].y, x[u].z, x[u].w};
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if ((j + q < N) & (e[q] > ninf) & topk_before(e[q], col0 + j + q, thr_v, thr_i)) m |= 1u << (u * 4 + q);
    }
    if (m) {
      int pos = atomicAdd(c, __popc(m));                           // pos + popc(m) <= TOPK_CHUNK: one slot per column of the chunk
#pragma unroll
      for (int u = 0; u < TOPK_VEC; ++u) {
        const int j = base + (u * TOPK_THREADS + tid) * 4;
        const float e[4] = {x[u].x, x[u].y, x[u].z, x[u].w};
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (m & (1u << (u * 4 + q))) { cv[pos] = e[q]; ci[pos] = col0 + j + q; ++pos; }
      }
    }
    __syncthreads();
    int n = *c;
    if (n == 0) continue;                                          // block-uniform

    int n2 = 1;
    while (n2 < n) n2 <<= 1;                                       // <= TOPK_CHUNK, a power of two
    for (int t = tid; t < n2; t += TOPK_THREADS) {
      bool drop = t >= n;
      if (!drop && f_hi > f_lo) {
        const int id = ci[t];
        int lo = f_lo, hi = f_hi;
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (filt_ids[mid] < id) lo = mid + 1; else hi = mid; }
        drop = lo < f_hi && filt_ids[lo] == id && id != kp;
      }
      if (drop) { cv[t] = ninf; ci[t] = -1; }
    }
    __syncthreads();
    float* lv1 = lv + (cur ^ 1) * TEMP_TOPK_MAX;                   // the list buffer that is not current: scratch until the merge fills it
    int* li1 = li + (cur ^ 1) * TEMP_TOPK_MAX;
    if (n > TOPK_PRUNE_MIN) {                                      // block-uniform
      float ev[TOPK_OWN], mv = ninf;
      int ei[TOPK_OWN], mi = -1;
#pragma unroll
      for (int i = 0; i < TOPK_OWN; ++i) {
        const int t = tid + i * TOPK_THREADS;
        ev[i] = t < n ? cv[t] : ninf;
        ei[i] = t < n ? ci[t] : -1;
        if (topk_before(ev[i], ei[i], mv, mi)) { mv = ev[i]; mi = ei[i]; }
      }
      lv1[tid] = mv;
      li1[tid] = mi;
      if (tid == 0) { *c = 0; cnt[2] = __float_as_int(ninf); cnt[3] = -1; }   // (every lane has read n before the barrier above)
      __syncthreads();
      int rank = 0;
      for (int j = 0; j < TOPK_THREADS; ++j) rank += topk_before(lv1[j], li1[j], mv, mi);
      if (mi >= 0 && rank == k - 1) { cnt[2] = __float_as_int(mv); cnt[3] = mi; }   // real bests have distinct keys: at most one lane
      __syncthreads();
      const float tv = __int_as_float(cnt[2]);
      const int ti = cnt[3];                                       // empty (fewer than k real bests): nothing comes after it
      unsigned live = 0;
#pragma unroll
      for (int i = 0; i < TOPK_OWN; ++i)
        if (ei[i] >= 0 && !topk_before(tv, ti, ev[i], ei[i])) live |= 1u << i;
      if (live) {
        int pos = atomicAdd(c, __popc(live));
#pragma unroll
        for (int i = 0; i < TOPK_OWN; ++i)
          if (live & (1u << i)) { cv[pos] = ev[i]; ci[pos] = ei[i]; ++pos; }
      }
      __syncthreads();
      n = *c;                                                      // T and what comes before it (0: the filter blanked everything)
      n2 = 1;
      while (n2 < n) n2 <<= 1;
      for (int t = n + tid; t < n2; t += TOPK_THREADS) { cv[t] = ninf; ci[t] = -1; }
      __syncthreads();
    }
    for (int size = 2; size <= n2; size <<= 1) {
      for (int stride = size >> 1; stride > 0; stride >>= 1) {
        for (int t = tid; t < (n2 >> 1); t += TOPK_THREADS) {
          const int a = ((t & ~(stride - 1)) << 1) | (t & (stride - 1)), b = a + stride;
          const float av = cv[a], bv = cv[b];
          const int ai = ci[a], bi = ci[b];
          const bool swap = (a & size) ? topk_before(av, ai, bv, bi) : topk_before(bv, bi, av, ai);
          if (swap) { cv[a] = bv; ci[a] = bi; cv[b] = av; ci[b] = ai; }
        }
        __syncthreads();
      }
    }
    float* lv0 = lv + cur * TEMP_TOPK_MAX;
    int* li0 = li + cur * TEMP_TOPK_MAX;
    if (tid == 0) *c = 0;                                          // every lane has read it; next appended to two chunks on
    const int ns = n2 < k ? n2 : k;                                // a survivor behind k others of its own chunk is out
    if (tid < k) {
      const float v = lv0[tid];
      const int id = li0[tid];
      const int np = tid + topk_count_before(cv, ci, ns, v, id);
      if (np < k) { lv1[np] = v; li1[np] = id; }
    }
    for (int t = tid; t < ns; t += TOPK_THREADS) {
      const float v = cv[t];
      const int id = ci[t];
      if (id < 0) continue;                                        // blanked or padding: sorted behind every survivor
      const int np = t + topk_count_before(lv0, li0, k, v, id);
      if (np < k) { lv1[np] = v; li1[np] = id; }
    }
    __syncthreads();
    cur ^= 1;
    thr_v = lv1[k - 1];
    thr_i = li1[k - 1];
  }
  if (tid < k) {
    top_val[out + tid] = lv[cur * TEMP_TOPK_MAX + tid];
    top_idx[out + tid] = li[cur * TEMP_TOPK_MAX + tid];
  }
}

}  // namespace
}  // namespace temp

using namespace temp;

namespace {

// the argument checks of both entry points (include/temp_amd.h); TEMP_OK with *launch = false for P == 0
int topk_check(int P, int N, int ld, int k, int col0, const float* a, const float* b, const float* w, bool mix, const float* top_val,
               const int32_t* top_idx, bool* launch) {
  *launch = false;
  if (P < 0 || N <= 0 || ld < N || k < 1 || k > TEMP_TOPK_MAX || col0 < 0 || (long long)col0 + N > 0x7fffffffLL) return TEMP_E_BADARG;
  if (ld % 4) return TEMP_E_UNSUPPORTED;
  if (P == 0) return TEMP_OK;
  if (!a || !top_val || !top_idx || (mix && (!b || !w))) return TEMP_E_BADARG;
  if (reinterpret_cast<uintptr_t>(a) % 16 || (mix && reinterpret_cast<uintptr_t>(b) % 16)) return TEMP_E_UNSUPPORTED;
  *launch = true;
  return TEMP_OK;
}

}  // namespace

extern "C" {

int temp_filtered_topk(int P, int N, int ld, int k, int col0, const float* scores, const int32_t* filt_ptr, const int32_t* filt_ids,
                       const int32_t* keep, int carry, float* top_val, int32_t* top_idx, void* stream) {
  bool launch;
  const int rc = topk_check(P, N, ld, k, col0, scores, nullptr, nullptr, false, top_val, top_idx, &launch);
  if (!launch) return rc;
  TEMP_LAUNCH(K_FILTERED_TOPK, k_filtered_topk<false>, dim3(P), dim3(TOPK_THREADS), TOPK_LDS, (hipStream_t)stream, N, ld, k, col0, scores,
              filt_ptr, filt_ids, keep, carry, top_val, top_idx, (const float*)nullptr, (const float*)nullptr);
  return launch_status();
}

int temp_filtered_topk_mix(int P, int N, int ld, int k, int col0, const float* scores_a, const float* scores_b, const float* w,
                           const int32_t* filt_ptr, const int32_t* filt_ids, const int32_t* keep, int carry, float* top_val,
                           int32_t* top_idx, void* stream) {
  bool launch;
  const int rc = topk_check(P, N, ld, k, col0, scores_a, scores_b, w, true, top_val, top_idx, &launch);
  if (!launch) return rc;
  TEMP_LAUNCH(K_FILTERED_TOPK_MIX, k_filtered_topk<true>, dim3(P), dim3(TOPK_THREADS), TOPK_LDS, (hipStream_t)stream, N, ld, k, col0, scores_a,
              filt_ptr, filt_ids, keep, carry, top_val, top_idx, scores_b, w);
  return launch_status();
}

}  // extern "C"
