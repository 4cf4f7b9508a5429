/*
 * temp_amd.h -- C ABI of the MI355X-native TeMP snapshot-encoder hot path (libtemp_amd.so).
 *
 * The TeMP reference (JiapengWu/TeMP) is pure Python and has no plugin / FFI layer; the seam this
 * library plugs into is the `ent_encoder` object installed by `build_model()`
 * (models/TKG_Module.py:37, models/DynamicRGCN.py:32-33, models/BiDynamicRGCN.py:14-15,
 * baselines/StaticRGCN.py:14-18).  Each entry point below names the reference code it replaces.
 * The Python mirror of the reference interface (package temp_amd) binds these symbols with ctypes;
 * INTEGRATION.md shows the stub a reference maintainer would add.
 *
 * Conventions
 *   - All arithmetic is fp32; all indices are int32; all matrices are dense row-major.
 *   - Every pointer is a DEVICE pointer unless stated otherwise.  The caller owns every buffer,
 *     including workspaces; the library never allocates or frees device memory and never synchronises
 *     (temp_rgcn_bwd / temp_rgcn_table_bwd order one side-stream branch against the caller's stream with two
 *     events, TEMP_OPT_OVERLAP: all of its work is complete, in stream order, when the call's last launch is).
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  The device is whatever
 *     is current in the calling thread.
 *   - Return value: 0 on success, a TEMP_E_* code otherwise (temp_error_string() describes it).
 *     Nothing is thrown across the ABI.  All functions are re-entrant (no global mutable state
 *     apart from the explicit switches of temp_set_option() and the bench-only trace),
 *     so forward may run on one thread and backward on PyTorch's autograd thread.
 *   - "nullable" arguments may be NULL.
 *   - Arithmetic of the dense products (TEMP_OPT_MFMA_BF16X3 = 1, the default): a product C = A . B whose row count (summed
 *     over the problems of one launch) is >= 16 384 runs on the bf16 matrix pipe as six products of an exact three-way split of
 *     both fp32 operands (fp32-equivalent accuracy: the dropped terms are below one fp32 rounding per product); below that
 *     row count the same call runs on the fp32 MFMA instructions.  The two agree to fp32 rounding, not bit for bit, so the
 *     same layer is bit-different on either side of the 16 384-row line; within one shape every result is bitwise repeatable.
 *     Non-finite inputs: the fp32 kernels propagate them as IEEE arithmetic does.  In the split kernels a non-finite operand
 *     (either side) makes every output that depends on it NON-FINITE -- NaN where fp32 arithmetic may give +-inf: the infinite
 *     piece of the split meets zero pieces of the other operand (inf . 0) -- and leaves all other outputs bit-identical.
 *     Round 6 (TEMP_OPT_MFMA_F16X2 = 1, the default): where an operand arrives with MAGNITUDE KEYS (the *_keys entry points below;
 *     a key = the fp32 bits of a row's / column's largest magnitude with the sign cleared) -- or the product is wide or deep enough
 *     to pay for taking them (N >= 512 or K >= 400) -- the same product runs on the f16 matrix pipe as THREE products of a two-way
 *     split of operands scaled by powers of two (csrc/split_f16.hpp).  Same accuracy class (<= 1e-6 of sum |a||b| against fp64,
 *     tests/test_gpu_f16_split.py), same non-finite contract; an element more than 2^17 below its row's (column's) largest keeps an
 *     ABSOLUTE error of 2^-39 of that largest value instead of a relative one.  Keys handed in must BOUND their row / column (a
 *     key that is too small overflows f16: the outputs of that row / column become non-finite).
 */
#ifndef TEMP_AMD_H
#define TEMP_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TEMP_ABI_VERSION 2

enum {
  TEMP_OK = 0,
  TEMP_E_BADARG = 1,      /* NULL / negative / inconsistent argument                          */
  TEMP_E_UNSUPPORTED = 2, /* shape outside what the kernels implement (see each function)    */
  TEMP_E_WORKSPACE = 3,   /* workspace too small                                             */
  TEMP_E_LAUNCH = 4       /* hipLaunch / hipGetLastError failure                             */
};

enum { TEMP_ACT_NONE = 0, TEMP_ACT_RELU = 1 };
enum { TEMP_GRU_TORCH = 0,   /* nn.GRU single step, gates r,z,n          (models/RRGCN.py:72,84)   */
       TEMP_GRU_TYPE1 = 1 }; /* "type-1" GRUCell, r,z from hidden only   (models/GRU_cell.py:7-31) */

int temp_abi_version(void);
const char* temp_error_string(int code);

/* Process-wide kernel-selection switches (A/B runs and bit-comparisons in ONE process; every setting computes the
 * same result to fp32 accuracy).  Each is one relaxed atomic int, read at launch time: a set is seen by every launch
 * issued after it returns, on any thread.  Defaults below; the environment variable named on each line, read ONCE
 * when the library is loaded, overrides the default (kept for runs that cannot call into the library first).
 * temp_set_option returns the previous value, or -1 for an unknown key; temp_get_option -1 for an unknown key. */
enum {
  TEMP_OPT_MFMA_BF16X3 = 0, /* 1: large fp32 products on the 16-bit matrix pipes through an operand split with fp32-equivalent accuracy
                               (which split: TEMP_OPT_MFMA_F16X2);  0: every product on the fp32 MFMA kernels
                                                                                           [TEMP_MFMA=f32 -> 0]       default 1 */
  TEMP_OPT_TN_SPLIT = 1,    /* 1: weight-gradient blocks of 4 row tiles x (4+3) column tiles  [TEMP_TN_SPLIT=0 -> 0]  default 1 */
  TEMP_OPT_RGCN_SCALAR = 2, /* 1: wide-row edge kernels keep per-edge quantities in SGPRs     [TEMP_RGCN_SCALAR=0 -> 0] default 1 */
  TEMP_OPT_GEMM_STREAM = 3, /* 1: force the streaming row-panel GEMM instead of weights-resident [TEMP_GEMM_STREAM=1 -> 1] default 0 */
  TEMP_OPT_GRU_STREAM = 4,  /* 1: force the streaming GRU cell kernel                          [TEMP_GRU_STREAM=1 -> 1] default 0 */
  TEMP_OPT_RGCN_TILE = 5,   /* 1: aggregation and d/dh stage a member snapshot's rows in LDS when the graph carries member tables
                               2: the weight-gradient kernel too (slower at the measured shapes)
                               3: the weight-gradient kernel with the gradient rows in LDS and the x rows read through L2 (same
                                  bits as 2; no faster than the gather kernel at the measured shapes)
                               0: always gather through L2 (bit-identical results)             [TEMP_RGCN_TILE=<n>]    default 1 */
  TEMP_OPT_DEBUG = 6,       /* development ablations inside instrumented kernels; 0 (off) in every product run          default 0 */
  TEMP_OPT_OVERLAP = 7,     /* 1: a layer's backward launches the relation-weight gradient -- and, without dropout, the loop-weight
                               and bias gradients behind it -- on a library-owned side stream (fork / join events on the caller's
                               stream: a parallel branch under HIP-graph capture) so that they overlap the d/dh aggregation and
                               the self-loop product; 0: everything on the caller's stream
                                                                                               [TEMP_OVERLAP=0 -> 0]    default 1 */
  TEMP_OPT_GEMM_RESIDENT = 8, /* 1: large fp32 products with K <= 208 keep the packed weights of four column tiles resident in LDS and
                               stream row panels through them (gemm_bxr.hpp); 0: one row tile per block, weights staged per slab
                                                                                               [TEMP_GEMM_RESIDENT=0 -> 0] default 1 */
  TEMP_OPT_MFMA_F16X2 = 9,  /* (with TEMP_OPT_MFMA_BF16X3 = 1)  1: where a kernel exists, three f16 MFMA products of the scaled two-way
                               split (split_f16.hpp: per-row / per-column power-of-two scales, residual <= one fp32 rounding);
                               0: six bf16 MFMA products of the exact three-way split everywhere (gemm_bx.hpp)
                                                                                           [TEMP_MFMA=bf16x3 -> 0]    default 1 */
  TEMP_OPT_RGCN_PAIR = 10,  /* pair route of a table-fed layer (temp_rgcn_pair_fwd / _bwd).  Low two bits: 0 never, 1 where it pays
                               (n_edges >= TEMP_PAIR_MIN_RATIO * n_rel_rows * n_table), 2 wherever the shapes are supported.
                               Bit 2 (+4): the forward keeps the table route; bit 3 (+8): the backward keeps it.  Read by the
                               callers that choose between temp_rgcn_table_* and temp_rgcn_pair_* (the Python package), not
                               by the entry points themselves                                  [TEMP_RGCN_PAIR=<n>]    default 1 */
  TEMP_OPT_COUNT = 11
};
int temp_set_option(int key, int value);
int temp_get_option(int key);
/* Diagnostic: how often a launch found no scratch slot for its packed weights / k-slice partials (more than 8 busy streams
 * on one device) and took the scratch-free kernels instead.  0 in every supported configuration. */
long long temp_scratch_refused(void);
/* Diagnostic: launches of f16-split kernels (TEMP_OPT_MFMA_F16X2) so far in this process -- a test's proof that the product it
 * checked did not silently take the six-product bf16 route. */
long long temp_f16_launches(void);
/* Diagnostic: edge-kernel launches (aggregation, d/dh, d/dweight) that took the LDS-tiled path (TempMembers present, member fits). */
long long temp_tile_launches(void);
/* Diagnostic: calls of temp_rgcn_pair_fwd / temp_rgcn_pair_bwd that launched their kernels. */
long long temp_pair_launches(void);
/* Diagnostic: which dense-product kernel ran.  Every launch site of the dense-product dispatcher (launch_gemm_panel_multi behind
 * temp_linear*, the self-loop / isolated / GRU products; the two extra branches of temp_linear_multi; the single-product fp32
 * weight-gradient kernel behind temp_linear_tn -- not the several-products launch of temp_linear_tn_multi nor the split-operand
 * weight-gradient kernels) adds one to the cell [route][width] when it launches its kernel; the trace names all of them
 * k_gemm_panel<...> / k_gemm_tn.  `width` is the kernel's template width (0 for the routes that have none, always < 8).
 * temp_gemm_route_launches returns the launches so far in this process, -1 for a route or width outside the table. */
enum {
  TEMP_ROUTE_PANEL = 0,       /* k_gemm_panel<NT>: fp32 MFMA row panels                                   width NT = 1..4  */
  TEMP_ROUTE_WRES = 1,        /* k_gemm_wres<NTS>: fp32 MFMA, weights resident, every block walks all problems  NTS = 1..3  */
  TEMP_ROUTE_WRES_SPLIT = 2,  /* k_gemm_wres<NTS>, `split`: every block serves one problem                      NTS = 1..3  */
  TEMP_ROUTE_BXP = 3,         /* k_gemm_bxp<G>: bf16 x6, packed weights from a scratch slot                       G = 1..7  */
  TEMP_ROUTE_BX = 4,          /* k_gemm_bx<G, 0>: bf16 x6, the block splits B[k][n] itself                        G = 1..7  */
  TEMP_ROUTE_BX_T = 5,        /* k_gemm_bx<G, 1>: the same for B stored [n][k]                                    G = 1..7  */
  TEMP_ROUTE_HXP = 6,         /* k_gemm_hxp<G>: f16 x3, slab-staged                                               G = 1..7  */
  TEMP_ROUTE_BXR = 7,         /* k_gemm_bxr: bf16 x6, weights resident                                            width 0   */
  TEMP_ROUTE_HXR = 8,         /* k_gemm_hxr: f16 x3, weights resident                                             width 0   */
  TEMP_ROUTE_KSLICE = 9,      /* temp_linear_multi: k-slices of k_gemm_panel<1> + one reduction (K >= 4096)       width 0   */
  TEMP_ROUTE_LINEAR_T = 10,   /* temp_linear_multi: C^T = B . A^T on k_gemm_bxr (trans_b, N >= 2048); its launch also counts
                                 as TEMP_ROUTE_BXR                                                                width 0   */
  TEMP_ROUTE_TN_W7 = 11,      /* k_gemm_tn<NT, 7, 1>: fp32 weight gradient, 7-wave blocks                   NT = 1, 2, 4, 7 */
  TEMP_ROUTE_TN_W8 = 12,      /* k_gemm_tn<NT, 8, 1>                                                        NT = 1, 2, 4, 7 */
  TEMP_ROUTE_TN_SPLIT = 13,   /* k_gemm_tn<7, 8, 2>: 4 row tiles x (4 + 3) column tiles (TEMP_OPT_TN_SPLIT)        NT = 7   */
  TEMP_ROUTE_COUNT = 14
};
long long temp_gemm_route_launches(int route, int width);
/* Diagnostic: which edge kernel ran.  Every launch site of the RGCN edge-kernel dispatcher (csrc/rgcn_kernels.hip: launch_agg_tile,
 * launch_agg, run_agg, launch_dw_tile, launch_dw_hybrid, run_dw, launch_fixup -- behind temp_rgcn_fwd / _bwd / _bwd_dh /
 * _bwd_weights / _table_fwd / _table_bwd; the pair route's own kernels are not counted, its k_fixup launch is) adds one to the
 * cell [route][s] when it launches its kernel; the trace names all of them k_rgcn_agg<...> / k_rgcn_dw / k_fixup.  `s` is the block
 * size of the relation weights the kernel is instantiated for (1, 2 or 4), 0 for the routes that have none (generic, fix-up).
 * temp_rgcn_route_launches returns the launches so far in this process, -1 for a route or s outside the table. */
enum {
  /* aggregation (MODE_FWD, by-dst view) */
  TEMP_RGCN_FWD_TILE8 = 0,        /* k_rgcn_agg_t<S, FWD, unsigned char>: member rows in LDS, n_rel_rows <= 256        s = 1, 2, 4 */
  TEMP_RGCN_FWD_TILE16 = 1,       /* k_rgcn_agg_t<S, FWD, unsigned short>: the same, 16-bit relation ids               s = 1, 2, 4 */
  TEMP_RGCN_FWD_LDS_SCALAR = 2,   /* k_rgcn_agg_s<S, FWD, true>: relation table in LDS, per-edge scalars (D > 128)     s = 1, 2, 4 */
  TEMP_RGCN_FWD_LDS_PERMUTE = 3,  /* k_rgcn_agg<S, FWD, true>: relation table in LDS, lane groups                      s = 1, 2, 4 */
  TEMP_RGCN_FWD_SCALAR = 4,       /* k_rgcn_agg_s<S, FWD, false>: weights through L2 (D > 128)                         s = 1, 2, 4 */
  TEMP_RGCN_FWD_PERMUTE = 5,      /* k_rgcn_agg<S, FWD, false>                                                         s = 1, 2, 4 */
  TEMP_RGCN_FWD_GENERIC = 6,      /* k_rgcn_agg_generic<FWD>: any si, so                                               s = 0       */
  /* d/dh (MODE_DX, by-src view): the same kernels, transposed blocks */
  TEMP_RGCN_DX_TILE8 = 7,
  TEMP_RGCN_DX_TILE16 = 8,
  TEMP_RGCN_DX_LDS_SCALAR = 9,
  TEMP_RGCN_DX_LDS_PERMUTE = 10,
  TEMP_RGCN_DX_SCALAR = 11,       /* k_rgcn_agg_s<S, DX, false>: only for a table beyond 64 KB (relation runs)                     */
  TEMP_RGCN_DX_PERMUTE = 12,
  TEMP_RGCN_DX_GENERIC = 13,
  /* weight gradient (by-rel view) */
  TEMP_RGCN_DW_HYBRID = 14,       /* k_rgcn_dw_h<S>: gradient rows in LDS, x rows through L2 (TEMP_OPT_RGCN_TILE = 3)  s = 1, 2, 4 */
  TEMP_RGCN_DW_TILE = 15,         /* k_rgcn_dw_t<S>: both row sets in LDS (TEMP_OPT_RGCN_TILE = 2)                     s = 1, 2, 4 */
  TEMP_RGCN_DW_SCALAR = 16,       /* k_rgcn_dw_s<S> (D > 128)                                                          s = 1, 2, 4 */
  TEMP_RGCN_DW_PERMUTE = 17,      /* k_rgcn_dw<S>                                                                      s = 1, 2, 4 */
  TEMP_RGCN_DW_GENERIC = 18,      /* k_rgcn_dw_generic                                                                 s = 0       */
  /* fix-up of the segments that span several chunks (any view) */
  TEMP_RGCN_FIX_FEW = 19,         /* k_fixup<16, 1, 32>: at most 1 024 (entry, column block) items                     s = 0       */
  TEMP_RGCN_FIX_MANY = 20,        /* k_fixup<4, 4, 256>                                                                s = 0       */
  TEMP_RGCN_FIX_FEW_SPLIT = 21,   /* k_fixup<16, 1, 32, true>: views of 32 768 and more partial rows                   s = 0       */
  TEMP_RGCN_FIX_MANY_SPLIT = 22,  /* k_fixup<4, 4, 256, true>                                                          s = 0       */
  TEMP_RGCN_FIX_SPLIT2 = 23,      /* k_fixup_split: second level behind either split launch                            s = 0       */
  TEMP_RGCN_ROUTE_COUNT = 24
};
long long temp_rgcn_route_launches(int route, int s);
/* Diagnostic: which per-position GRU cell kernel ran.  The forward kernels all trace as k_gru_fwd and every instantiation of the
 * gate-gradient kernel as k_gru_bwd_gates; each launch site of csrc/gru_kernels.hip (launch_gru_fwd_wres, launch_gru_fwd_batch,
 * temp_gru_cell_fwd_multi's zero-state launch, launch_gru_gates_batch) adds one to its route when it launches its kernel.  The
 * weights-resident forward also counts as (TEMP_ROUTE_WRES_SPLIT, 3) of temp_gemm_route_launches.
 * temp_gru_route_launches returns the launches so far in this process, -1 for a route outside the table. */
enum {
  TEMP_GRU_FWD_WRES = 0,            /* k_gemm_wres<3, EpiGruCell<V>>: hoisted gates, d % 8 == 0, three gate tiles fit 80 KB of LDS */
  TEMP_GRU_FWD_STREAM_HOISTED = 1,  /* k_gru_fwd<V, true>: hoisted gates, the widths the resident kernel refuses, TEMP_OPT_GRU_STREAM */
  TEMP_GRU_FWD_STREAM_FUSED = 2,    /* k_gru_fwd<V, false>: x . W_ih^T computed inside (temp_gru_fwd)                              */
  TEMP_GRU_FWD_ZERO = 3,            /* k_gru_fwd_zero<V>: cells of temp_gru_cell_fwd_multi whose prev is NULL                      */
  TEMP_GRU_GATES_LPR8 = 4,          /* k_gru_bwd_gates<V, 8>: d <= 32                                                              */
  TEMP_GRU_GATES_LPR16 = 5,         /* k_gru_bwd_gates<V, 16>: d <= 64                                                             */
  TEMP_GRU_GATES_LPR32 = 6,         /* k_gru_bwd_gates<V, 32>: d <= 128                                                            */
  TEMP_GRU_GATES_LPR64 = 7,         /* k_gru_bwd_gates<V, 64>: wider (a lane makes a second pass beyond d = 256)                   */
  TEMP_GRU_ROUTE_COUNT = 8
};
long long temp_gru_route_launches(int route);
/* Development only: a device buffer of `words` int64 into which instrumented kernels write cycle-counter stamps (NULL: off).
 * The edge kernels stamp 8 words per block into its first 32768 words (launches of more than 4096 blocks do not stamp).  A buffer of
 * 32768 + 4096 words or more also switches the f16 chain launchers to their stamped instantiations, which write words 32768 .. 36863
 * (csrc/gru_chain_hx.hpp: CHX_STAMP_WORDS; tools/chain_phases.py reads them); a smaller buffer leaves the chain kernels as they are.
 * Not used by the product path. */
void temp_set_debug_buffer(void* device_ptr, size_t words);

/* ------------------------------------------------------------------------------------------------
 * Segmented edge lists.  One batched snapshot graph (the disjoint union `dgl.batch` builds at
 * models/DynamicRGCN.py:92) is handed over as three sorted views of the same E edges, each cut
 * into chunks of at most TEMP_CHUNK edges (TEMP_CHUNK_REL for the by-relation view, whose segments
 * are few and long) that never straddle a segment:
 *
 *   by destination  (forward aggregation,  RGCNLayer.propagate  models/RGCN.py:100-104)
 *   by source       (d/dh of the aggregation)
 *   by relation     (d/dweight of the aggregation, RGCNLayer.msg_func models/RGCN.py:91-98)
 *
 * A view holds, per edge in sorted order, the two "other" attributes (`a`, `b`), and per chunk the
 * segment id (node or relation row), its [beg,end) edge range and a partial-result slot:
 *   slot == -1 : the chunk is the whole segment, its result is final;
 *   slot >= 0  : the segment spans several chunks; this chunk's partial goes to partial slot `slot`
 *                and `fix_*` lists every such segment with its first slot and slot count (slots of
 *                one segment are consecutive and are summed in order => deterministic).
 * ---------------------------------------------------------------------------------------------- */
#define TEMP_CHUNK 64
#define TEMP_CHUNK_REL 128

/* Dropout of the self-loop message (RGCNLayer.forward, models/RGCN.py:57-59; the reference's default --dropout is 0.1).
 * The keep mask is a counter-based hash of (seed, node row, output column), so forward and backward regenerate the
 * same mask and nothing is stored:  loop_message[row, col] *= (hash(seed, row, col) < p) ? 0 : 1 / (1 - p).
 * A NULL TempDropout* (or p == 0) means no dropout. */
typedef struct TempDropout {
  float p;
  uint64_t seed;
} TempDropout;

typedef struct TempEdgeView {
  int32_t n_seg;            /* number of segments (nodes, or relation rows)                        */
  int32_t n_edges;          /* E                                                                   */
  const int32_t* a;         /* [E]  by-dst: src node   | by-src: dst node | by-rel: src node       */
  const int32_t* b;         /* [E]  by-dst: relation   | by-src: relation | by-rel: dst node       */
  int32_t n_chunks;
  const int32_t* chunk_seg; /* [n_chunks]                                                          */
  const int32_t* chunk_beg; /* [n_chunks]                                                          */
  const int32_t* chunk_end; /* [n_chunks]                                                          */
  const int32_t* chunk_slot;/* [n_chunks]                                                          */
  int32_t n_partial;        /* total partial slots                                                 */
  int32_t n_fix;            /* segments that span more than one chunk                              */
  const int32_t* fix_seg;   /* [n_fix]                                                             */
  const int32_t* fix_slot;  /* [n_fix] first slot                                                  */
  const int32_t* fix_cnt;   /* [n_fix] number of slots                                             */
} TempEdgeView;

/* Optional member tables of a batched graph (the disjoint union `dgl.batch` builds, models/DynamicRGCN.py:92): the union's
 * nodes, the edge arrays of every view and the chunk lists of every view are MEMBER-MAJOR (member m owns the node rows
 * [node_off[m], node_off[m+1]), positions [edge_off[m], edge_off[m+1]) of every view's a/b arrays and chunks
 * [chunk_off[v][m], chunk_off[v][m+1]) of view v = 0 by_dst, 1 by_src, 2 by_rel; no edge crosses members).  With them the edge
 * kernels run one workgroup per (member, feature slice) with the member's rows staged in LDS (block-diagonal relation weights
 * make feature slices independent) instead of gathering rows through L2 -- same chunks, same summation order, bit-identical
 * results.  n_members == 0 (or a member too large for LDS): the kernels gather from global memory as before. */
typedef struct TempMembers {
  int32_t n_members;
  int32_t max_nodes;        /* largest member: nodes                                               */
  int32_t max_edges;        /*                 edge-array positions (edge_off[m+1] - edge_off[m])  */
  int32_t max_chunks[3];    /*                 chunks in the by_dst / by_src / by_rel view         */
  const int32_t* node_off;  /* [n_members + 1]  device                                             */
  const int32_t* edge_off;  /* [n_members + 1]  device                                             */
  const int32_t* chunk_off; /* [3][n_members + 1] device                                           */
  const int32_t* fix_off;   /* [2][n_members + 1] device, nullable: first fix-up entry of every member in the by_dst / by_src
                               view (their fix_* lists are member-major).  Present: the LDS-tiled aggregation / d-dh kernels sum
                               a member's multi-chunk segments themselves, after their walk (one launch less per view). */
} TempMembers;

typedef struct TempGraph {
  int32_t n_nodes;          /* sum of nodes over the batched snapshots                             */
  int32_t n_edges;
  const float* nnorm;       /* [n_nodes] 1/in_degree, 0 for in_degree 0 (utils/utils.py:74-79)     */
  const int32_t* in_deg;    /* [n_nodes]                                                           */
  const int32_t* out_deg;   /* [n_nodes]                                                           */
  TempEdgeView by_dst;
  TempEdgeView by_src;      /* needed by temp_rgcn_bwd only                                        */
  TempEdgeView by_rel;      /* needed by temp_rgcn_bwd only; n_seg = number of weight rows (2R)    */
  TempMembers members;      /* optional (n_members = 0: absent)                                    */
} TempGraph;

/* ------------------------------------------------------------------------------------------------
 * RGCN layer  (RGCNLayer.forward, models/RGCN.py:53-76, dropout = 0)
 *
 *   out[v] = act( nnorm[v]^2 * sum_{(u,r) in In(v)} h[u] . BD(W[r])  [+ bias]  +  h[v] . loop_w )
 *
 * BD(W[r]) is the block-diagonal matrix of `num_bases` blocks of (si x so), si = d_in/num_bases,
 * so = d_out/num_bases, stored row-major per block (b*si*so + i*so + o) -- the `.view(-1, si, so)`
 * of models/RGCN.py:92-93.  The double normalisation (edge norm then node norm) is the
 * reference's.  `h_ids` (nullable) fuses the embedding gather of
 * models/DynamicRGCN.py:93: row v of the input is h[h_ids[v]].
 * Supported: d_in == d_out, d_in % 4 == 0, si == so in {1,2,4} (fast path) or any si,so
 * (generic path).  workspace >= temp_rgcn_fwd_workspace().
 * ---------------------------------------------------------------------------------------------- */
size_t temp_rgcn_fwd_workspace(const TempGraph* g, int d_out);
int temp_rgcn_fwd(const TempGraph* g, const float* h, const int32_t* h_ids /*nullable*/,
                  int d_in, int d_out, int num_bases, int n_rel_rows,
                  const float* weight, const float* loop_w, const float* bias /*nullable*/, int act,
                  float* out, void* workspace, size_t workspace_bytes, const TempDropout* drop, void* stream);

/* Backward of the above (autograd of models/RGCN.py:53-104).
 *   d_h      [n_nodes, d_in]   written (not accumulated)
 *   d_weight [n_rel_rows, num_bases*si*so]  written; rows of unused relations are zeroed
 *   d_loop_w [d_in, d_out]     written
 *   d_bias   [d_out]           written (nullable iff bias was NULL)
 * `out` is the forward output (used for the ReLU mask only when act == TEMP_ACT_RELU).
 * `h` must be the materialised [n_nodes, d_in] input (no fused gather in backward). */
size_t temp_rgcn_bwd_workspace(const TempGraph* g, int d_in, int d_out, int num_bases, int n_rel_rows);
int temp_rgcn_bwd(const TempGraph* g, const float* h, const float* out, const float* d_out_grad,
                  int d_in, int d_out, int num_bases, int n_rel_rows,
                  const float* weight, const float* loop_w, int has_bias, int act,
                  float* d_h, float* d_weight, float* d_loop_w, float* d_bias /*nullable*/,
                  void* workspace, size_t workspace_bytes, const TempDropout* drop, void* stream);

/* The two halves of temp_rgcn_bwd, for a layer INSIDE a recurrence (the reference's default flags: both layers recurrent,
 * models/RRGCN.py:179-204): d_h position by position, the weight gradients once over the union of all positions' graphs.
 *   temp_rgcn_bwd_dh:      d_h [n_nodes, d_in] only.  act == TEMP_ACT_RELU: the ReLU-masked gradient is written to dz_out
 *                          [n_nodes, d_out] (required then); with dropout the masked gradient of the self-loop message is written
 *                          to dzm_out (required then).  act == TEMP_ACT_NONE without dropout: both may be NULL (dz = d_out_grad).
 *   temp_rgcn_bwd_weights: d_weight / d_loop_w / d_bias from h [n_nodes, d_in], dz (the masked gradient) and dzm (NULL: = dz) --
 *                          the same kernels temp_rgcn_bwd runs, on whatever graph the rows belong to (a union of positions).
 * Workspace: temp_rgcn_bwd_workspace of the graph. */
int temp_rgcn_bwd_dh(const TempGraph* g, const float* out /*nullable unless relu*/, const float* d_out_grad, int d_in, int d_out, int num_bases,
                     int n_rel_rows, const float* weight, const float* loop_w, int act, float* d_h, float* dz_out /*nullable*/,
                     float* dzm_out /*nullable*/, void* workspace, size_t workspace_bytes, const TempDropout* drop, void* stream);
int temp_rgcn_bwd_weights(const TempGraph* g, const float* h, const float* dz, const float* dzm /*nullable*/, int d_in, int d_out, int num_bases,
                          int n_rel_rows, int has_bias, float* d_weight, float* d_loop_w, float* d_bias /*nullable*/, void* workspace,
                          size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Same layer when its input is a ROW GATHER of a table, h = table[ids]  (layer 1 of every TeMP encoder:
 * g.ndata['h'] = ent_embeds[g.ndata['id']], models/DynamicRGCN.py:93).  h is never materialised:
 *   fwd: the aggregation gathers through ids; the self-loop term is (table . W_loop)[ids] -- one N_table-row GEMM
 *        instead of one over every node row of the batch;
 *   bwd: what is linear in the gathered rows is summed per table row first (inv_ptr / inv_order = the ids grouped
 *        by table row, see temp_segment_sum_rows):  d_table = segsum(d_h_agg) + segsum(dz) . W_loop^T  [n_table, d_in]
 *        (fully written, deterministic), d_loop_w = table^T . segsum(dz).
 * Results equal temp_rgcn_fwd/bwd on h = table[ids] followed by the gather's adjoint, up to fp32 summation order.
 * ---------------------------------------------------------------------------------------------- */
size_t temp_rgcn_table_fwd_workspace(const TempGraph* g, int n_table, int d_out);
int temp_rgcn_table_fwd(const TempGraph* g, const float* table, const int32_t* ids, int n_table, int d_in, int d_out, int num_bases,
                        int n_rel_rows, const float* weight, const float* loop_w, const float* bias, int act, float* out, void* workspace,
                        size_t workspace_bytes, const TempDropout* drop, void* stream);
size_t temp_rgcn_table_bwd_workspace(const TempGraph* g, int n_table, int d_in, int d_out, int num_bases);
int temp_rgcn_table_bwd(const TempGraph* g, const float* table, const int32_t* ids, const int32_t* inv_ptr, const int32_t* inv_order, int n_table,
                        const float* out, const float* d_out_grad, int d_in, int d_out, int num_bases, int n_rel_rows, const float* weight,
                        const float* loop_w, int has_bias, int act, float* d_table, float* d_weight, float* d_loop_w, float* d_bias,
                        void* workspace, size_t workspace_bytes, const TempDropout* drop, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Pair route of the table-fed layer.  The message of an edge (u, r, v) of a layer whose input is table[ids] is
 * table[ids[u]] . BD(W[r]): it depends on the PAIR (r, ids[u]) only, not on the snapshot or the destination.  When a graph has
 * many more edges than the n_rel_rows * n_table pairs (a union of many snapshots over a small entity set: GDELT), the block
 * products run once per pair and the edge passes become plain row gathers:
 *   fwd:  M[r, e] = table[e] . BD(W[r])                                 P = n_rel_rows * n_table rows
 *         out[v]  = act( nnorm[v]^2 * sum_{(u,r) in In(v)} M[r, ids[u]]  [+ bias]  +  drop((table . W_loop)[ids[v]]) )
 *   bwd:  G[r, e] = sum over the edges (u, r, v) with ids[u] = e of nnorm[v]^2 * dz[v]
 *         d_table[e] = sum_r G[r, e] . BD(W[r])^T + (segsum(dzm) . W_loop^T)[e],   d_W[r] = sum_e table[e]^T (x) G[r, e] blockwise
 * Every sum runs in a fixed order (no atomics): results are bitwise repeatable and equal temp_rgcn_table_fwd / _bwd up to fp32
 * summation order.
 *
 * TempPairView is built once per (graph, ids) by the caller (temp_amd/pair_view.py), on the device:
 *   fwd_row [by_dst.n_edges]: per position of the by_dst view's edge arrays the row of M it reads, b * n_table + ids[a]
 *                             (positions that no chunk covers -- a device-subsampled member -- are never read)
 *   by_pair: the edges grouped by pair in a reproducible order (stable sort of the by_dst positions by pair), as a
 *            TempEdgeView: a = destination node, b unused (may be NULL), chunks of at most TEMP_CHUNK_PAIR edges with ordered
 *            partial slots, n_seg = P + 1.  EVERY pair owns at least one chunk (an empty one for a pair without edges: its G
 *            row is written as zeros).  The lists are sized from upper bounds so that no count has to reach the host:
 *            trailing chunks are { seg = P, beg = end, slot = -1 } and trailing fix entries { seg = P, cnt = 0 }; row P of
 *            G absorbs them.  n_partial bounds the slots in use.
 * temp_expand_chunk_segments: seg_of[p] = chunk_seg[c] for every position p in [chunk_beg[c], chunk_end[c]) of a view, -1 for
 * positions no chunk covers (seg_of: [n_pos], fully written) -- the per-edge segment ids the builder sorts by.
 * Supported (temp_rgcn_pair_supported): d_in == d_out, d % 4 == 0, d <= 256, si == so in {1, 2, 4}; else TEMP_E_UNSUPPORTED.
 * ---------------------------------------------------------------------------------------------- */
#define TEMP_CHUNK_PAIR 128
#define TEMP_PAIR_MIN_RATIO 4
typedef struct TempPairView {
  int32_t n_table;
  int32_t n_rel_rows;
  const int32_t* fwd_row;
  TempEdgeView by_pair;
} TempPairView;
int temp_expand_chunk_segments(int n_chunks, const int32_t* chunk_seg, const int32_t* chunk_beg, const int32_t* chunk_end, int n_pos,
                               int32_t* seg_of, void* stream);
int temp_rgcn_pair_supported(int d_in, int d_out, int num_bases);
size_t temp_rgcn_pair_fwd_workspace(const TempGraph* g, const TempPairView* pv, int d_out);
int temp_rgcn_pair_fwd(const TempGraph* g, const TempPairView* pv, const float* table, const int32_t* ids, int n_table, int d_in, int d_out,
                       int num_bases, int n_rel_rows, const float* weight, const float* loop_w, const float* bias, int act, float* out,
                       void* workspace, size_t workspace_bytes, const TempDropout* drop, void* stream);
size_t temp_rgcn_pair_bwd_workspace(const TempGraph* g, const TempPairView* pv, int d_in, int d_out, int num_bases);
int temp_rgcn_pair_bwd(const TempGraph* g, const TempPairView* pv, const float* table, const int32_t* ids, const int32_t* inv_ptr,
                       const int32_t* inv_order, int n_table, const float* out, const float* d_out_grad, int d_in, int d_out, int num_bases,
                       int n_rel_rows, const float* weight, const float* loop_w, int has_bias, int act, float* d_table, float* d_weight,
                       float* d_loop_w, float* d_bias, void* workspace, size_t workspace_bytes, const TempDropout* drop, void* stream);

/* Isolated-entity variant (RGCNLayer.forward_isolated, models/RGCN.py:78-89):
 *   out = act( e + e . loop_w [+ bias] )          e: [n, d]                                    */
int temp_rgcn_isolated_fwd(int n, int d, const float* e, const float* loop_w, const float* bias /*nullable*/,
                           int act, float* out, const TempDropout* drop, void* stream);
size_t temp_rgcn_isolated_bwd_workspace(int n, int d);
int temp_rgcn_isolated_bwd(int n, int d, const float* e, const float* out, const float* d_out_grad,
                           const float* loop_w, int has_bias, int act,
                           float* d_e, float* d_loop_w, float* d_bias /*nullable*/,
                           void* workspace, size_t workspace_bytes, const TempDropout* drop, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Recurrent update: decay of the previous state + one GRU step
 * (GRRGCNLayer.forward, models/RRGCN.py:77-89; BiGRRGCNLayer, models/BiRRGCN.py:27-63).
 *
 *   hdec[i] = prev[prev_idx ? prev_idx[i] : i] * exp(-lambda * dt[i])                (fixed)
 *           = prev[...] * exp(-max(0, decay_w * dt[i] + decay_b))                    (learnable,
 *                                                     RGCNLayer.decay_hidden models/RGCN.py:106-107)
 *   prev_idx[i] == -1  =>  previous state is the zero vector (entity inactive at the previous
 *                          window position: the reference re-zeroes its dense history every step,
 *                          models/DynamicRGCN.py:47-54).
 *   TEMP_GRU_TORCH:  r = sig(W_ir x + b_ir + W_hr hdec + b_hr),  z likewise,
 *                    n = tanh(W_in x + b_in + r * (W_hn hdec + b_hn)),  h' = (1-z) n + z hdec
 *                    w_ih, w_hh: [3d, d] rows ordered r,z,n;  b_ih, b_hh: [3d]
 *   TEMP_GRU_TYPE1:  r = sig(W_hr hdec + b_hr), z = sig(W_hz hdec + b_hz),
 *                    n = tanh(W_in x + b_in + r * (W_hn hdec + b_hn)),  h' = n + z (hdec - n)
 *                    w_ih: [d, d], b_ih: [d];  w_hh: [3d, d], b_hh: [3d]
 *   `learnable`: decay_wb points to 2 DEVICE floats {w, b}; otherwise decay_wb is NULL and
 *   `lambda` is used.
 *   saved: [5, n, d] scratch the backward needs (r, z, n, W_hn hdec + b_hn, hdec).
 * Supported: d % 4 == 0.
 * ---------------------------------------------------------------------------------------------- */
int temp_gru_fwd(int n, int d, int variant,
                 const float* x, const float* prev, const int32_t* prev_idx /*nullable*/, const float* dt,
                 float lambda, const float* decay_wb /*nullable*/,
                 const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh,
                 float* h_out, float* saved, void* stream);

/* Backward.  d_h_out: [n,d] upstream gradient.
 *   d_x    [n,d]  written
 *   d_prev [n,d]  written, in the row order of x (caller scatters through prev_idx)
 *   d_w_ih, d_w_hh, d_b_ih, d_b_hh written
 *   d_decay_wb: 2 device floats written when learnable (nullable otherwise)                       */
size_t temp_gru_bwd_workspace(int n, int d, int variant);
int temp_gru_bwd(int n, int d, int variant,
                 const float* x, const float* prev, const int32_t* prev_idx /*nullable*/, const float* dt,
                 float lambda, const float* decay_wb /*nullable*/,
                 const float* w_ih, const float* w_hh,
                 const float* saved, const float* d_h_out,
                 float* d_x, float* d_prev, float* d_w_ih, float* d_w_hh, float* d_b_ih, float* d_b_hh,
                 float* d_decay_wb /*nullable*/,
                 void* workspace, size_t workspace_bytes, void* stream);

/* Fixed exponential decay as a stand-alone row scale: out[r, :] = x[r, :] * exp(-dt[r] * lambda) -- the recurrent term of the
 * linear-recurrence layers (RRGCNLayer models/RRGCN.py:130-151, BiRRGCNLayer models/BiRRGCN.py:115-140), whose GEMM runs through
 * temp_linear.  Self-adjoint (the backward is the same call on the gradient).  out may alias x. */
int temp_decay_rows(int n, int d, const float* x, const float* dt, float lambda, float* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Window-batched recurrence.  When only the last layer is recurrent (--rec-only-last-layer,
 * models/RRGCN.py:182-187) the GRU input x of EVERY window position is known before the chain
 * starts, so everything that is not truly sequential is hoisted out of the per-position loop:
 *
 *   temp_gru_input_gates   gi = x . W_ih^T + b_ih for all positions at once  (one MFMA GEMM)
 *   temp_gru_cell_fwd      per position: hdec . W_hh^T on MFMA + gates + blend (reads its gi rows)
 *   temp_gru_cell_bwd      per position: gate gradients + d_prev = (dgh . W_hh + dh*z) * decay;
 *                          the gradient arriving from the NEXT position is gathered through the
 *                          inverse row map `next_idx` (-1 = none) and added to `dh_up` (nullable)
 *   temp_gru_weight_grads  after the chain: d_x = dgi . W_ih, d_W_ih = dgi^T x, d_W_hh = dgh^T hdec,
 *                          bias column sums -- over ALL rows that share one set of GRU weights
 *
 * `saved` planes (r, z, n, W_hn hdec + b_hn, hdec) are `saved_plane` floats apart so that every
 * position writes its rows into one [5, N_total, d] buffer and `hdec` (plane 4) is contiguous for
 * the batched weight gradient.  gi/dgi: [n, 3d] (torch) or [n, d] (type-1); dgh: [n, 3d]; decv: [n].
 * Fixed decay only (learnable decay uses temp_gru_fwd / temp_gru_bwd).
 * ---------------------------------------------------------------------------------------------- */
int temp_gru_input_gates(int n, int d, int variant, const float* x, const float* w_ih, const float* b_ih, float* gi, void* stream);
/* The same for `count` (row block, weight set) pairs of one width in as few launches as possible (four problems each): the input
 * gates of both directions of a bidirectional window chain (models/BiRRGCN.py:206-221: forward_rnn and backward_rnn).  Results
 * are bit-identical to `count` calls of temp_gru_input_gates. */
int temp_gru_input_gates_multi(int count, const int* ns, int d, int variant, const float* const* xs, const float* const* w_ihs,
                               const float* const* b_ihs, float* const* gis, void* stream);
/* ... with the rows of problem i gathered: gis[i] row j = xs[i][x_idx[i][j]] . W_ih^T + b_ih (x_idx: HOST array of device int32
 * tables, an entry may be NULL = rows in order; indices >= 0).  Used to compute the gates of every DISTINCT input row of a
 * window chain once (TempGruChain.gi_index maps chain rows to gi rows).  Within one arithmetic (Conventions: the 16 384-row
 * switch looks at the rows of the whole launch) a row's result does not depend on where it is computed: gates[gi_index[i]] is then bit-identical to
 * temp_gru_input_gates_multi's row i. */
int temp_gru_input_gates_gather_multi(int count, const int* ns, int d, int variant, const float* const* xs, const int32_t* const* x_idx,
                                      const float* const* w_ihs, const float* const* b_ihs, float* const* gis, void* stream);
int temp_gru_cell_fwd(int n, int d, int variant, const float* gi, const float* prev, const int32_t* prev_idx /*nullable*/,
                      const float* dt, float lambda, const float* w_hh, const float* b_hh,
                      float* h_out, float* saved, size_t saved_plane, void* stream);
int temp_gru_cell_bwd(int n, int d, int variant, const float* saved, size_t saved_plane,
                      const float* dh_up /*nullable*/, const float* d_prev_next /*nullable*/, const int32_t* next_idx /*nullable*/,
                      const float* dt, float lambda, const float* w_hh,
                      float* dgi, float* dgh, float* decv, float* d_prev, void* stream);
/* Several independent cells in ONE launch each (forward chain and backward chain of the bidirectional
 * window advance position by position together; count <= 4; arrays are HOST arrays of structs). */
typedef struct TempGruCellFwd {
  int32_t n; const float* gi; const float* prev /* NULL: the cell starts from the zero state (pointwise, no GEMM) */;
  const int32_t* prev_idx /*nullable*/; const float* dt;
  const float* w_hh; const float* b_hh; float* h_out; float* saved /* first row of the cell inside the [5, N, d] planes */;
} TempGruCellFwd;
typedef struct TempGruCellBwd {
  int32_t n; const float* saved; const float* dh_up /*nullable*/; const float* d_prev_next /*nullable*/;
  const int32_t* next_idx /*nullable*/; const float* dt; const float* w_hh;
  float* dgi; float* dgh; float* decv; float* d_prev;
  int32_t no_prev;   /* != 0: the cell started from a zero state (first position of a chain): nothing consumes d_prev, so its
                        GEMM is skipped and d_prev is left holding only the gate kernel's seed */
} TempGruCellBwd;
int temp_gru_cell_fwd_multi(int count, const TempGruCellFwd* cells, int d, int variant, float lambda, size_t saved_plane, void* stream);
int temp_gru_cell_bwd_multi(int count, const TempGruCellBwd* cells, int d, int variant, float lambda, size_t saved_plane, void* stream);
size_t temp_gru_weight_grads_workspace(int n, int d, int variant);
/* hdec may be NULL when every row started from the zero state (d_w_hh = 0, d_b_hh = column sums of dgh). */
int temp_gru_weight_grads(int n, int d, int variant, const float* x, const float* hdec, const float* dgi, const float* dgh,
                          const float* w_ih, float* d_x /*nullable*/, float* d_w_ih, float* d_w_hh, float* d_b_ih, float* d_b_hh,
                          void* workspace, size_t workspace_bytes, void* stream);
/* The same for `count` <= 4 GRUs of one width in ONE weight-gradient launch + ONE reduction + ONE d_x launch (both directions of a
 * bidirectional window chain, models/BiRRGCN.py:206-221): d_w = [2 count, 3d, d] holds d_W_ih_0, d_W_hh_0, d_W_ih_1, ...,
 * d_b = [2 count, 3d] the bias gradients in the same order; xs / hdecs / dgis / dghs / w_ihs / d_xs are HOST arrays of device
 * pointers (a d_xs entry may be NULL).  nn.GRU gate layout only; TEMP_E_UNSUPPORTED (nothing launched) for shapes that need the
 * per-GRU call (type-1 cell, small row counts, a GRU whose rows all start from the zero state: hdecs[i] NULL).  Same sums as the
 * per-GRU call up to the order of the row slices. */
size_t temp_gru_weight_grads_multi_workspace(int count, const int* ns, int d, int variant);
int temp_gru_weight_grads_multi(int count, const int* ns, int d, int variant, const float* const* xs, const float* const* hdecs,
                                const float* const* dgis, const float* const* dghs, const float* const* w_ihs, float* const* d_xs,
                                float* d_w, float* d_b, void* workspace, size_t workspace_bytes, void* stream);

/* Weight / bias gradients and d_x of `count` <= 4 GRUs from their gate-gradient matrices g4s[i] = [ns[i]][4d] (temp_gru_chain_bwd's g4):
 *   d_W_ih = [dr dz dn_i]^T x,  d_W_hh = [dr dz dn_h]^T hdec,  d_b_* = the column sums,  d_x = [dr dz dn_i] . W_ih
 * (the backward of the GRU step, models/RRGCN.py:84) -- ONE weight-gradient launch (k_gru_wgrad: both products of every GRU read
 * their columns of the one matrix through a column map; the row-wise sums take their fragments through LDS transpose reads, no
 * operand is turned in registers), ONE deterministic reduction over the row slices, ONE d_x launch.  Output layout as
 * temp_gru_weight_grads_multi: d_w = [2 count][3d][d] (d_W_ih_0, d_W_hh_0, d_W_ih_1, ...), d_b = [2 count][3d].  xs / hdecs / g4s /
 * w_ihs / d_xs: HOST arrays of device pointers (a d_xs entry may be NULL).  The workspace query returns 0 and the call
 * TEMP_E_UNSUPPORTED (nothing launched) for shapes that take the dgi / dgh calls: d % 8 != 0, d >= 256, fewer than 16 384
 * rows in all, TEMP_OPT_MFMA_BF16X3 off.  fp32-equivalent arithmetic (six bf16 MFMA products of the exact operand split). */
size_t temp_gru_grads_g4_workspace(int count, const int* ns, int d);
int temp_gru_grads_g4(int count, const int* ns, int d, const float* const* xs, const float* const* hdecs, const float* const* g4s,
                      const float* const* w_ihs, float* const* d_xs, float* d_w, float* d_b, void* workspace, size_t workspace_bytes,
                      void* stream);
/* Round 6: the same with the keys temp_gru_chain_bwd hands out (HOST arrays of `count` device pointers; NULL arrays or
 * TEMP_OPT_MFMA_F16X2 = 0: exactly temp_gru_grads_g4).  g4_col_keys[i]: [4d] keys bounding the column magnitudes of g4s[i];
 * g4_row_keys[i]: [ns[i]] keys of the rows' max |[dr dz dn_i]|.  With them the products run as three f16 MFMA products of the
 * scaled two-way split (split_f16.hpp) instead of six bf16 products; hdecs must be decayed GRU states (|hdec| < 4: they are split
 * with the constant scale 2^14).  Same workspace. */
int temp_gru_grads_g4_keys(int count, const int* ns, int d, const float* const* xs, const float* const* hdecs, const float* const* g4s,
                           const float* const* w_ihs, float* const* d_xs, float* d_w, float* d_b, const uint32_t* const* g4_row_keys,
                           const uint32_t* const* g4_col_keys, const uint32_t* const* x_col_keys /* nullable (array or entries): [d] keys
                           bounding the column magnitudes of xs[i], e.g. from temp_gather_rows_keys; else taken here with one pass */,
                           void* workspace, size_t workspace_bytes, void* stream);
/* temp_gru_grads_g4_keys with the GRUs' input rows read IN PLACE: row m of GRU i's x is table[x_rows[i][m]] (table: [table_rows][d];
 * x_rows: HOST array of `count` device int32 lists of ns[i] entries, each 0 <= r < table_rows -- not checked on the device).  No
 * copy of the rows in GRU order is needed (k_gru_wgrad_hx_rows forms each staged row's offset from its entry, loaded ahead of the
 * row).  The keys are required, x_col_keys[i] included (keys bounding the table's columns bound any selection of its rows); the
 * results equal temp_gru_grads_g4_keys on the gathered copy with the same keys bit for bit.  d_xs as there (GRU row order).
 * TEMP_E_UNSUPPORTED (nothing launched) where temp_gru_grads_g4_rows_supported returns 0: shapes temp_gru_grads_g4 refuses,
 * TEMP_OPT_MFMA_F16X2 = 0, table_rows . d . 4 or ns[i] . d . 4 >= 2^32 (32-bit lane offsets), or a row slice whose row list does not
 * fit LDS behind the slab buffers (more than about 14 000 rows per slice: GRUs of several hundred thousand rows).  Same workspace. */
int temp_gru_grads_g4_rows_supported(int count, const int* ns, int d, int table_rows);
int temp_gru_grads_g4_rows(int count, const int* ns, int d, const float* table, int table_rows, const int32_t* const* x_rows,
                           const float* const* hdecs, const float* const* g4s, const float* const* w_ihs, float* const* d_xs, float* d_w,
                           float* d_b, const uint32_t* const* g4_row_keys, const uint32_t* const* g4_col_keys,
                           const uint32_t* const* x_col_keys, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Persistent window chain: ALL positions of the recurrence in ONE launch per direction of time.
 *
 * The recurrence of the window models is per (window, direction, entity): a row at position p reads only the state of the
 * SAME entity at position p-1 (`prev_idx`; models/DynamicRGCN.py:35-54, models/RRGCN.py:77-89).  So the rows of a chain
 * program split into independent *panels* of <= 32 entity tracks; a workgroup owns a panel, keeps its 32 states in LDS and
 * walks all positions of the chain without ever meeting another workgroup: no grid barrier, no relaunch.  Per position a
 * panel does  hdec . W_hh^T  (32 x 3d x d) on the fp32 MFMA pipe with W_hh streamed from L2 in fragment order
 * (temp_gru_chain_pack), then the gates / blend pointwise; the backward walks the positions in reverse with
 * d_prev = (dgh . W_hh + dh*z) * decay kept in LDS.  Replaces 15 x (temp_gru_cell_fwd_multi) and
 * 15 x (temp_gru_cell_bwd_multi) launches of a seq_len-15 bidirectional window.
 *
 * Tables (device, int32), built once per prepared batch on the host:
 *   panel [n_panels][4] : { GRU index (< n_rnn), first step (row of the step tables), number of steps, 0 }
 *   rows  [S][32]       : per step and track: row in the [N_total, *] buffers | TEMP_CHAIN_HAS_PREV if the track carries a
 *                         state from the step before (else the state is zero), or -1 (track idle at this step)
 *   sinfo [S][4]        : { flags (bit0: some track of the step has a previous state, bit1: write h_out rows),
 *                           up: index into `up` of the upstream gradient block of the step's rows or -1,
 *                           up_row0: first row of that block in the [N_total] row space, 0 }
 * Steps of a panel are consecutive table rows in chain order.  gi / saved / dgi / dgh / h: as for temp_gru_cell_*.
 * The previous state of a row with time gap dt is scaled by exp(-dt lambda) (c->lambda), or by a learnable decay (c->decay); a state
 * offset (c->offset) is added behind the cell.  d % 4 == 0 and d <= TEMP_CHAIN_MAX_D (LDS), else TEMP_E_UNSUPPORTED.
 * ---------------------------------------------------------------------------------------------- */
#define TEMP_CHAIN_HAS_PREV (1 << 30)
#define TEMP_CHAIN_TRACKS 32
#define TEMP_CHAIN_MAX_RNN 4
#define TEMP_CHAIN_MAX_UP 8
/* Learnable decay (--learnable-lambda; RGCNLayer.decay_hidden, models/RGCN.py:106-107): exp(-max(w dt + b, 0)) instead of
 * exp(-dt lambda); c->lambda is not read.  wb[i]: DEVICE {w, b} of GRU i (no host read, no sync: capturable); GRUs may share one pair. */
typedef struct TempChainDecay { const float* wb[TEMP_CHAIN_MAX_RNN]; } TempChainDecay;
/* State offset (--use-time-embedding; models/RRGCN.py:192-204, models/BiRRGCN.py:228-240): the state a row hands on is
 *   s_rho = GRU(x_rho, dec . s_prev) + table[index[rho]]
 * -- the add follows the cell and becomes part of the recurrent state, so |s| is not bounded by 1.  table: DEVICE [n_rows][d], shared
 * by all GRUs of the chain (layer_2.time_embed); index: DEVICE int32 [N_total], an entry outside [0, n_rows) (-1) = no offset.
 * Pointers only, no host read: capturable.  Composes with either decay.
 *   Layout: the f16 kernels (TEMP_CHAIN_PACK_HX, _HX_X) split the state with the constant scale 2^14, which needs |state| < 4: an
 *     offset chain runs on the TEMP_CHAIN_PACK_BX kernels (exact three-way bf16 split, any range), or _F32 where d % 8 != 0 or the
 *     bf16 route is off.  temp_gru_chain_offset_layout(d) names that layout; temp_gru_chain_pack_multi_layout writes it.
 *   Forward: h_out and the state kept for the next position are the sum; saved[4] stays the decayed previous state (now
 *     dec . s_prev), so the gate arithmetic and the weight gradients are those of a chain without offset.  Consumers of saved[4] must
 *     not assume |hdec| < 4 (temp_gru_grads_g4, not _g4_keys). */
typedef struct TempChainOffset { const float* table; const int32_t* index; int32_t n_rows; } TempChainOffset;
typedef struct TempGruChain {
  int32_t d, variant, n_panels, n_steps;
  int32_t max_steps;                     /* longest panel (<= 64): sizes the per-panel tables the kernels stage in LDS */
  const int32_t* panel; const int32_t* rows; const int32_t* sinfo;
  const float* dt;                       /* [N_total] time gap of every row */
  float lambda;
  size_t saved_plane;
  int32_t n_rnn;
  const float* packed[TEMP_CHAIN_MAX_RNN];   /* temp_gru_chain_pack of each GRU's W_hh */
  const float* b_hh[TEMP_CHAIN_MAX_RNN];
  const int32_t* gi_index;               /* nullable [N_total]: row of `gi` that holds row i's input gates.  Chain rows that read the
                                          * same input row share one gi row (temp_gru_input_gates_gather_multi computes each once);
                                          * NULL: gi has N_total rows, row i's gates in row i.  Forward only: dgi stays per row. */
  int32_t pack_layout;                   /* TEMP_CHAIN_PACK_*: the layout `packed` was written in -- temp_gru_chain_pack_layout(d) at the
                                          * time of temp_gru_chain_pack / _pack_multi, TEMP_CHAIN_PACK_HX_X for temp_gru_chain_pack_x_multi.
                                          * The kernels follow it (not the options at launch time); a layout this width cannot have:
                                          * TEMP_E_BADARG. */
  const TempChainDecay* decay;           /* nullable: NULL = the fixed c->lambda */
  const TempChainOffset* offset;         /* nullable: NULL = no state offset */
} TempGruChain;
enum { TEMP_CHAIN_PACK_F32 = 1, TEMP_CHAIN_PACK_BX = 2, TEMP_CHAIN_PACK_HX = 3, TEMP_CHAIN_PACK_HX_X = 4 };
/* the layout temp_gru_chain_pack / _pack_multi write for width d under the current options (TEMP_OPT_MFMA_*) */
int temp_gru_chain_pack_layout(int d);
int temp_gru_chain_supported(int d);
size_t temp_gru_chain_pack_floats(int d);                                   /* floats of one packed W_hh */
int temp_gru_chain_pack(int d, const float* w_hh, float* packed, void* stream);
/* count <= TEMP_CHAIN_MAX_RNN matrices in one launch (w_hh / packed: HOST arrays of device pointers; each packed[i] holds
 * temp_gru_chain_pack_floats(d) floats), in the layout temp_gru_chain_pack_layout(d) names / in a given layout (F32 / BX / HX) */
int temp_gru_chain_pack_multi(int count, int d, const float* const* w_hh, float* const* packed, void* stream);
int temp_gru_chain_pack_multi_layout(int layout, int count, int d, const float* const* w_hh, float* const* packed, void* stream);
/* x route: W_hh laid out as temp_gru_chain_pack_multi lays it out (the backward takes the same buffer), followed by W_ih's planes */
size_t temp_gru_chain_pack_x_floats(int d);
int temp_gru_chain_pack_x_multi(int count, int d, const float* const* w_hh, const float* const* w_ih, float* const* packed, void* stream);
/* The forward.  gi route: the input gates `gi` (c->gi_index applies).  x route (x != NULL): the input gates computed inside (nn.GRU
 * gate layout, f16 arithmetic) -- x [x rows][d], x_index [N_total]: x row of chain row i, b_ih: HOST array of n_rnn device pointers,
 * c->packed[i] from temp_gru_chain_pack_x_multi; no gate GEMM.  h_out / saved as temp_gru_cell_fwd (saved[4] = the decayed state). */
typedef struct TempChainFwd {
  const float* gi; const float* x; const int32_t* x_index; const float* const* b_ih;
  float* h_out; float* saved;
} TempChainFwd;
int temp_gru_chain_fwd(const TempGruChain* c, const TempChainFwd* io, void* stream);
/* The backward.  up: HOST array of n_up device pointers (sinfo's `up`).  Three output routes:
 *   gates (g4 == NULL): dgi and dgh, as temp_gru_cell_bwd.
 *   g4 (nn.GRU gate layout only): the gate gradients written ONCE, g4 [n_rows][4d] = [dr | dz | dn_i | dn_h] -- dgi = columns
 *     0 .. 3d-1, dgh = columns 0 .. 2d-1 and 3d .. 4d-1 (two thirds of dgh repeated dgi).  Bit-identical values; for temp_gru_grads_g4.
 *   g4 with keys (each nullable; HX / HX_X packs only): also what temp_gru_grads_g4_keys needs to split g4 for the f16 pipe --
 *     row_keys [N_total]: per row the largest magnitude of [dr dz dn_i] as an unsigned key (the fp32 bits with the sign cleared;
 *       integer order = magnitude order)
 *     col_keys [n_rnn + n_panels][4d]: rows 0 .. n_rnn - 1 = per GRU and column of g4 a key that BOUNDS the column's largest magnitude
 *       (integer maxima: order-independent, bit-repeatable); the n_panels rows behind them are scratch (every panel's own maxima,
 *       reduced by a second small launch); no initialisation needed
 * d_arg [N_total] (exactly with c->decay) = dL / d(w dt + b) of every row that has a previous state (0 where the clamp is active; the
 *   other rows are not written):  d_arg[rho] = -[w dt_rho + b > 0] <d_prev_rho, h_pi>,  pi = the row of the same track one position earlier.
 * d_state [N_total][d] (nullable, only with c->offset): the total gradient reaching every row's state (upstream + d_prev of its
 *   successor; ds/dh = I, so the gate gradients are unchanged), every row written once with plain stores.  d_table is then the adjoint
 *   of the row gather table[index] applied to d_state (temp_gather_rows' backward with a static inverse): no atomics, bit-repeatable. */
typedef struct TempChainBwd {
  const float* saved; int32_t n_up; const float* const* up;
  float* dgi; float* dgh; float* g4; uint32_t* row_keys; uint32_t* col_keys;
  float* d_arg; float* d_state;
} TempChainBwd;
int temp_gru_chain_bwd(const TempGruChain* c, const TempChainBwd* io, void* stream);
/* Return contract of both calls, checked in this order; nothing is launched on an error:
 *   1. descriptor -- NULL c / io, sizes, variant, n_rnn, max_steps, a NULL packed[i] / b_hh[i]: BADARG; a width the chain does not
 *      take: UNSUPPORTED; a pack_layout the width cannot have: BADARG
 *   2. c->decay -- a NULL wb[i]: BADARG; not temp_gru_chain_decay_supported: UNSUPPORTED
 *   3. c->offset -- NULL table / index, n_rows <= 0: BADARG; not temp_gru_chain_offset_supported, or HX / HX_X packs: UNSUPPORTED
 *   4. route, BADARG -- both gi and x; x with pack_layout != HX_X; d_state without c->offset; n_up outside [0, TEMP_CHAIN_MAX_UP] or
 *      n_up > 0 with up NULL; (c->decay != NULL) != (d_arg != NULL); g4 together with dgi or dgh; row_keys / col_keys without g4
 *      route, UNSUPPORTED -- x with the type-1 cell or a panel too long for its LDS images; g4 with the type-1 cell (its dgi is
 *      [n, d]); keys with packs other than HX / HX_X (hence keys with an offset)
 *   5. n_panels == 0: TEMP_OK;  6. only then a NULL buffer of the route (gi | x, x_index, b_ih[i]; h_out; saved; dgi, dgh | g4): BADARG
 * "Both gi and x" and "keys without g4" are stricter than the per-feature entries before this pair (inexpressible / ignored there).
 * temp_gru_chain_fwd_x_supported: 1 when callers should take the x route (the f16 route is selected, the LDS images fit this width
 *   and max_steps, TEMP_DEBUG bit 22 -- the A/B switch to the gi route -- is clear).  temp_gru_chain_keys_supported: 1 when the
 *   kernels of this width produce keys (f16 arithmetic selected and its LDS images fit).
 * temp_gru_chain_{fwd_x,decay,offset}_launches (diagnostic, since the library was loaded): launches of the x route's kernel; chain
 *   forward / backward launches with a learnable decay; with an offset. */
int temp_gru_chain_fwd_x_supported(int d, int variant, int max_steps);
long long temp_gru_chain_fwd_x_launches(void);
int temp_gru_chain_keys_supported(int d);
int temp_gru_chain_decay_supported(int d, int variant);
long long temp_gru_chain_decay_launches(void);
int temp_gru_chain_offset_supported(int d, int variant);
int temp_gru_chain_offset_layout(int d);
long long temp_gru_chain_offset_launches(void);
/* d_wb [n_rnn][2] = per GRU { sum d_arg dt, sum d_arg } over its rows with a previous state, in a fixed order (per-panel partials in
 * `ws`, temp_gru_chain_decay_reduce_workspace(c) bytes; no atomics: bit-repeatable).  Reads c's tables and n_rnn only. */
size_t temp_gru_chain_decay_reduce_workspace(const TempGruChain* c);
int temp_gru_chain_decay_reduce(const TempGruChain* c, const float* d_arg, float* d_wb, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Persistent window chain of the LINEAR recurrence (--module RRGCN / BiRRGCN; models/RRGCN.py:120-167, models/BiRRGCN.py:102-185):
 *   hdec[rho] = exp(-lambda dt[rho]) . h[pi]            (0 without TEMP_CHAIN_HAS_PREV; pi = the row of the same track one step earlier)
 *   h[rho]    = act(x[x_index ? x_index[rho] : rho] + hdec[rho] . W_i)        W_i stored (in, out), i = panel[.][0]
 * ALL positions in ONE launch on TempGruChain's tables (panel / rows / sinfo as described there, read unchanged): a workgroup owns a
 * panel of TEMP_CHAIN_TRACKS tracks, keeps their states in LDS and walks its steps.  Per step one 32 x d x d product on the fp32 MFMA
 * pipe, W_i streamed from L2 in fragment order (temp_lin_chain_pack_multi: `count` <= TEMP_CHAIN_MAX_RNN matrices in one launch, w /
 * packed HOST arrays of device pointers, temp_lin_chain_pack_floats(d) floats each).  fp32 arithmetic throughout: the state is not bounded.
 * The decay is applied BEFORE the product (BiRRGCNLayer.forward's order; RRGCNLayer applies it behind: the same value up to rounding).
 *   forward:  EVERY row of h and hdec [N_total][d] is written (sinfo's write flag is not read: the backward needs all of h and the
 *             weight gradient all of hdec).
 *   backward: positions in reverse.  g = the upstream block of the step (sinfo's up / up_row0; up: HOST array of n_up device pointers,
 *             a NULL entry = no gradient for that block) + d_prev handed back by the successor;  d_pre[rho] = g . [h[rho] > 0] (act = 1)
 *             or g (act = 0), every row written;  d_prev of pi = dec(rho) . (d_pre[rho] . W_i^T), kept in LDS.
 *             d_pre is d_x (through the adjoint of x_index) and the left factor of d_W_i = hdec_i^T . d_pre_i over weight i's rows
 *             (temp_linear_tn / _multi).  No atomics, one reduction order per launch shape: bit-repeatable.
 * Device pointers only, no host read: capturable.  Return contract of _fwd / _bwd, in this order; nothing is launched on an error:
 *   NULL c, d <= 0, negative counts, n_w outside 1 .. TEMP_CHAIN_MAX_RNN, act outside {0, 1}, a NULL packed[i], NULL tables or
 *   max_steps == 0 with n_panels > 0: BADARG;  d % 4 != 0, d > TEMP_CHAIN_MAX_D or max_steps > 64: UNSUPPORTED;  (bwd) n_up outside
 *   0 .. TEMP_CHAIN_MAX_UP or n_up > 0 with up NULL: BADARG;  n_panels == 0: TEMP_OK without a launch;  then a NULL x / h / hdec / d_pre:
 *   BADARG.  temp_lin_chain_launches (diagnostic): forward + backward launches since the library was loaded.
 * ---------------------------------------------------------------------------------------------- */
#define TEMP_CHAIN_MAX_D 256
typedef struct TempLinChain {
  int32_t d, n_panels, n_steps, max_steps;
  const int32_t* panel; const int32_t* rows; const int32_t* sinfo;   /* TempGruChain's tables; panel[.][0] = weight index */
  const float* dt; float lambda;                                    /* [N_total]; dec = exp(-dt lambda) */
  int32_t n_w; const float* packed[TEMP_CHAIN_MAX_RNN];             /* temp_lin_chain_pack_multi of each W (in, out) */
  int32_t act;                                                      /* 0 none, 1 ReLU */
} TempLinChain;
int temp_lin_chain_supported(int d, int max_steps);
size_t temp_lin_chain_pack_floats(int d);
int temp_lin_chain_pack_multi(int count, int d, const float* const* w, float* const* packed, void* stream);
int temp_lin_chain_fwd(const TempLinChain* c, const float* x, const int32_t* x_index /* nullable [N_total] */,
                       float* h /* [N_total][d] */, float* hdec /* [N_total][d] */, void* stream);
int temp_lin_chain_bwd(const TempLinChain* c, const float* h, int32_t n_up, const float* const* up /* HOST array */,
                       float* d_pre /* [N_total][d] */, void* stream);
long long temp_lin_chain_launches(void);
/* ONE position of the same recurrence on gathered rows, without the track tables (the (window, entity) pair rows of the batched
 * all-entity pass, where both layers of --module RRGCN are recurrent):
 *   fwd:  hdec[i] = exp(-lambda dt[i]) H[h_rows[i]]   (0 where h_rows[i] < 0);   out[i] = act(x[x_rows ? x_rows[i] : i] + hdec[i] . W)
 *         (a negative x_rows[i] reads a zero row);
 *   bwd:  d_pre[i] = up[i] . [out[i] > 0] (act = 1) or up[i];   d_hrows[i] = exp(-lambda dt[i]) (d_pre[i] . W^T)   (0 where h_rows[i] < 0).
 * A workgroup of 256 threads owns 32 rows and runs the chain's three phases once (gather + decay, the 32 x d x d fp32 MFMA product, the
 * epilogue); fp32 throughout, the decay in front of the product as in the chain; no atomics, one summation order: bit-repeatable.  All
 * n rows of out, hdec, d_pre and d_hrows are written.  pack_fwd / pack_bwd: the first / second half of W's temp_lin_chain_pack_multi
 * buffer (temp_lin_chain_pack_floats(d) / 2 floats each).  The caller finishes the backward: d_H and d_x are the segment sums of
 * d_hrows / d_pre through the inverses of h_rows / x_rows, d_W = hdec^T . d_pre (temp_linear_tn).  Device pointers only: capturable.
 * Return contract, in this order; nothing is launched on an error: n < 0, d <= 0 or act outside {0, 1}: BADARG;  a width
 * temp_lin_rows_supported refuses (temp_lin_chain_supported's rule): UNSUPPORTED;  n == 0: TEMP_OK without a launch;  then a NULL
 * x / H / h_rows / dt / pack / out / hdec (fwd), up / h_rows / dt / pack / d_pre / d_hrows or, with act = 1, out (bwd): BADARG. */
int temp_lin_rows_supported(int d);
int temp_lin_rows_fwd(int n, int d, const float* x, const int32_t* x_rows /* nullable [n] */, const float* H, const int32_t* h_rows /* [n] */,
                      const float* dt /* [n] */, float lambda, const float* pack_fwd, int act, float* out /* [n][d] */, float* hdec /* [n][d] */,
                      void* stream);
int temp_lin_rows_bwd(int n, int d, const float* out, const float* up, const int32_t* h_rows, const float* dt, float lambda,
                      const float* pack_bwd, int act, float* d_pre /* [n][d] */, float* d_hrows /* [n][d] */, void* stream);
/* ONE position of the BIDIRECTIONAL linear recurrence on gathered rows (BiRRGCNLayer's centre position and the union (window, entity)
 * pair rows of its batched all-entity pass): both directions' recurrent terms in front of ONE activation.  For s in {f, b}:
 *   fwd:  hdec_s[i] = exp(-lambda dt_s[i]) H_s[rows_s[i]]   (0 where rows_s[i] < 0);
 *         out[i] = act(x[x_rows ? x_rows[i] : i] + hdec_f[i] . W_f + hdec_b[i] . W_b)   (a negative x_rows[i] reads a zero row);
 *   bwd:  d_pre[i] = up[i] . [out[i] > 0] (act = 1) or up[i];   d_hrows_s[i] = exp(-lambda dt_s[i]) (d_pre[i] . W_s^T)   (0 where rows_s[i] < 0).
 * temp_lin_rows' implementation with two history sources instead of one (one kernel template per direction of the step, instantiated
 * for both pairs of calls): a workgroup of 256 threads owns 32 rows and runs the three phases once.  The forward gathers and decays
 * both sources into LDS and accumulates both products into one accumulator set (a K = 2 d walk over [hdec_f | hdec_b] against the two
 * packed weights); the backward reads the one d_pre tile against W_f^T and against W_b^T.  fp32 throughout, the decay in front of the
 * product; no atomics, one summation order: bit-repeatable.  All n rows of out, hdec_f, hdec_b, d_pre, d_hrows_f and d_hrows_b are
 * written.  pack_fwd_s / pack_bwd_s: the first / second half of W_s's temp_lin_chain_pack_multi buffer.  The caller finishes the
 * backward: d_H_s and d_x are the segment sums of d_hrows_s / d_pre through the inverses of rows_s / x_rows, d_W_s = hdec_s^T . d_pre
 * (temp_linear_tn).  Device pointers only: capturable.  A direction without any state passes rows_s all -1 (H_s is then never read,
 * but must not be NULL).
 * Return contract, in this order; nothing is launched on an error: n < 0, d <= 0 or act outside {0, 1}: BADARG;  a width
 * temp_lin_rows2_supported refuses (temp_lin_chain_supported's rule: d % 4 == 0, d <= 256; 100 352 bytes of LDS at d = 256):
 * UNSUPPORTED;  n == 0: TEMP_OK without a launch;  then a NULL x / H_s / rows_s / dt_s / pack / out / hdec_s (fwd), up / rows_s / dt_s /
 * pack / d_pre / d_hrows_s or, with act = 1, out (bwd): BADARG. */
int temp_lin_rows2_supported(int d);
int temp_lin_rows2_fwd(int n, int d, const float* x, const int32_t* x_rows /* nullable [n] */, const float* H_f, const int32_t* rows_f /* [n] */,
                       const float* dt_f /* [n] */, const float* H_b, const int32_t* rows_b /* [n] */, const float* dt_b /* [n] */, float lambda,
                       const float* pack_fwd_f, const float* pack_fwd_b, int act, float* out /* [n][d] */, float* hdec_f /* [n][d] */,
                       float* hdec_b /* [n][d] */, void* stream);
int temp_lin_rows2_bwd(int n, int d, const float* out, const float* up, const int32_t* rows_f, const float* dt_f, const int32_t* rows_b,
                       const float* dt_b, float lambda, const float* pack_bwd_f, const float* pack_bwd_b, int act, float* d_pre /* [n][d] */,
                       float* d_hrows_f /* [n][d] */, float* d_hrows_b /* [n][d] */, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Row gather / scatter helpers of the window loop
 * (get_prev_embeddings / update_time_diff_hist_embeddings / ent_embeds[id],
 *  models/DynamicRGCN.py:35-54,93).
 *   gather:       out[i] = idx[i] >= 0 ? table[idx[i]] : 0                 out: [n, d]
 *   scatter_add:  table[idx[i]] += src[i]  for idx[i] >= 0 (atomic, rows may repeat)
 * ---------------------------------------------------------------------------------------------- */
int temp_gather_rows(int n, int d, const float* table, const int32_t* idx, float* out, void* stream);
/* Magnitude keys (round 6, split_f16.hpp): the key of a value is its fp32 bit pattern with the sign cleared, so integer order is
 * magnitude order and a maximum of keys does not depend on the order it is taken in.  A consumer that runs a product as three f16
 * MFMA products scales every row (activations) / column (a sum over rows) by the power of two its key gives.
 *   temp_absmax_keys      : row_keys[n] (nullable) = key of every row's largest magnitude; col_keys (nullable) = [d] keys bounding
 *                           every column's largest magnitude, followed by temp_keys_cols_size(d) - d words of scratch (the buffer
 *                           holds temp_keys_cols_size(d) words; nothing to initialise).  d % 4 == 0, d <= 256.
 *   temp_gather_rows_keys : temp_gather_rows that also hands out the keys of its OUTPUT rows / columns (same buffers).
 *   temp_linear_keys      : temp_linear with the row keys of A (nullable: taken inside when the product is wide or deep enough to pay
 *                           for the pass, else the six-product bf16 kernels run).
 *   temp_gru_input_gates_gather_multi_keys : x_keys[i] = row keys of xs[i] by source row (nullable array / entries). */
size_t temp_keys_cols_size(int d);
int temp_absmax_keys(int n, int d, const float* x, int ldx, uint32_t* row_keys, uint32_t* col_keys, void* stream);
int temp_gather_rows_keys(int n, int d, const float* table, const int32_t* idx, float* out, uint32_t* row_keys, uint32_t* col_keys, void* stream);
int temp_linear_keys(int M, int N, int K, const float* A, int lda, const uint32_t* a_keys, const float* B, int ldb, int trans_b, float* C, int ldc,
                     void* stream);
int temp_gru_input_gates_gather_multi_keys(int count, const int* ns, int d, int variant, const float* const* xs, const int32_t* const* x_idx,
                                           const uint32_t* const* x_keys, const float* const* w_ihs, const float* const* b_ihs, float* const* gis,
                                           void* stream);
int temp_scatter_add_rows(int n, int d, const float* src, const int32_t* idx, float* table, void* stream);
/* Deterministic adjoint of a gather with a STATIC index list (the ids of a prepared window batch):
 *   out[s] = sum_{j in [seg_ptr[s], seg_ptr[s+1])} src[order[j]]      out: [n_seg, d] fully written (empty segment = 0)
 * seg_ptr [n_seg+1] / order [n_rows] = the gather indices grouped by table row (built once on the host;
 * ids < 0 are left out, so n_rows may be smaller than the gather).  n_rows must be EXACTLY the length of `order`
 * (= seg_ptr[n_seg]): the piece kernels size their partials from it (a smaller value would drop the trailing rows).
 * No atomics; d % 4 == 0 (else TEMP_E_UNSUPPORTED).  d <= 256 takes the routes below; wider rows are summed by one wave per
 * segment, 256 columns at a time, whatever the segment lengths (workspace 0).  Tables with very long segments (>= 512 rows per segment on average, e.g. the
 * relation table under the loss) are reduced in two deterministic stages through `workspace`; segmentations of 2-32 rows per
 * segment on average are summed over fixed 32-row pieces of `order` (skew-proof: a hub entity's thousands of rows are many
 * pieces, not one wave's loop) with the piece partials in `workspace`
 * (temp_segment_sum_rows_workspace bytes; 0 for the other shapes; NULL falls back to one wave / one block per segment). */
size_t temp_segment_sum_rows_workspace(int n_seg, int n_rows, int d);
int temp_segment_sum_rows(int n_seg, int n_rows, int d, const int32_t* seg_ptr, const int32_t* order, const float* src, float* out,
                          void* workspace, size_t workspace_bytes, void* stream);
/* The same with the adjoint of a ReLU folded in: out[s][c] = relu_of[s][c] > 0 ? sum : 0, where relu_of [n_seg, d] is the
 * POST-activation table the gather read (y = relu(z) => y > 0 <=> z > 0).  For a gather that is the only consumer of an
 * RGCN layer's ReLU output (models/BiRRGCN.py:202-203 -> the GRU input rows), the layer's backward then takes the gradient as
 * already masked (act = TEMP_ACT_NONE) and the (n, d) mask pass of its own disappears. */
int temp_segment_sum_rows_relu(int n_seg, int n_rows, int d, const int32_t* seg_ptr, const int32_t* order, const float* src, const float* relu_of,
                               float* out, void* workspace, size_t workspace_bytes, void* stream);

/* The diachronic entity table (baselines/DiachronicEmbedding.py:22-28) for B timestamps at once, and its adjoint:
 *   out[(b N + j), c] = ent[j, c]                                             c <  ds = d / 2   (integer division)
 *                     = ent[j, c] * sin(t[b] * w[j, c - ds] + b[j, c - ds])   c >= ds
 * ent [N, d], w and b [N, d - ds], t [B] in DEVICE memory, out / d_out [B N, d].  The argument is formed as torch forms it -- the
 * product and the sum are two rounded fp32 operations, never a fused multiply-add -- and goes through the range-reducing
 * sinf / cosf (t w reaches the thousands).  The backward keeps nothing from the forward and OVERWRITES
 *   d_ent = sum_b d_out (1 | sin)      d_b = sum_b d_out ent cos      d_w = sum_b d_out ent cos t[b]
 * with the B terms added in ascending b in registers: no atomics, no workspace, one launch, bit-repeatable.
 * Any B >= 1, N >= 1, d >= 2 (else TEMP_E_BADARG): float4 on every stream when d % 4 == 0 and ds % 4 == 0, one column per thread
 * otherwise.  A pure stream: 2 N d floats read and B N d written forward, the mirror image backward. */
int temp_diachronic_rows_fwd(int B, int N, int d, const float* ent, const float* w, const float* b, const float* t, float* out, void* stream);
int temp_diachronic_rows_bwd(int B, int N, int d, const float* ent, const float* w, const float* b, const float* t, const float* d_out, float* d_ent,
                             float* d_w, float* d_b, void* stream);

/* The hyperplane projection of a table for B normals (HyTE, baselines/Hyte.py:18-27: every entity row and every relation row of
 * timestamp b is projected onto the hyperplane whose normal is that timestamp's time row), and its adjoint.  With n_b = w_b / |w_b|_2:
 *   out[b N + i, :] = table[i, :] - n_b (n_b . table[i, :])
 * table [N, d], w [B, d] (the B time rows, already gathered), out / d_out [B N, d], all 16-byte aligned.  One launch: the normals
 * are normalised inside it (each wave forms them from w, TEMP_HYPERPLANE_CHUNK = 8 at a time in registers; a table row is read once
 * per chunk, i.e. once for B <= 8), a stream of N d floats read and B N d written.
 * The backward keeps nothing from the forward and OVERWRITES, with G = d_out,
 *   d_table[i] = sum_b (G_bi - n_b (n_b . G_bi))                              the B terms added in ascending b
 *   d_n_b      = -sum_i [(n_b . e_i) G_bi + (n_b . G_bi) e_i]                 e_i = table[i]
 *   d_w_b      = (d_n_b - n_b (n_b . d_n_b)) / |w_b|
 * in two launches and without floating-point atomics.  The sum over i runs over FIXED tiles of TEMP_HYPERPLANE_TILE_ROWS = 32
 * consecutive rows (tile t = rows [32 t, 32 t + 32) whatever the device or the grid): the first launch writes every tile's partial
 * of every normal into `workspace` ([tiles, B, d] floats, each written once: no zero fill), the second adds them in ascending
 * tile order and applies the normalisation Jacobian.  Results are bit-repeatable.
 *   workspace bytes = ceil(N / TEMP_HYPERPLANE_TILE_ROWS) * B * d * 4       (= temp_hyperplane_rows_bwd_workspace(B, N, d))
 * A smaller or NULL workspace returns TEMP_E_BADARG and launches nothing.  Any B >= 1, N >= 1, d >= 1 (else TEMP_E_BADARG):
 * float4 columns when d % 4 == 0, one float per lane otherwise; rows of more than 64 such columns are walked by a column loop.
 * A zero time row gives non-finite values, as the reference's division does. */
#define TEMP_HYPERPLANE_TILE_ROWS 32
#define TEMP_HYPERPLANE_CHUNK 8
size_t temp_hyperplane_rows_bwd_workspace(int B, int N, int d);
int temp_hyperplane_rows_fwd(int B, int N, int d, const float* table, const float* w, float* out, void* stream);
int temp_hyperplane_rows_bwd(int B, int N, int d, const float* table, const float* w, const float* d_out, float* d_table, float* d_w,
                             void* workspace, size_t workspace_bytes, void* stream);

/* The pair table of two tables for B windows (SimplE, baselines/Simple.py: every entity and every relation has a forward and an inverse
 * row), and its adjoint:
 *   out[b N + i, :] = [a[i, :] | a_inv[i, :]]                 b = 0 .. B - 1
 * a, a_inv [N, d], out / d_out [B N, 2 d] row-major.  One launch: a thread reads its columns of a and a_inv once and writes them B
 * times (2 N d floats read, 2 B N d written).  The backward OVERWRITES both outputs whole,
 *   d_a[i] = sum_b d_out[b N + i, :d],   d_a_inv[i] = sum_b d_out[b N + i, d:]        the B terms added in ascending b in fp32,
 * in one launch, without atomics and without a workspace: results are bit-repeatable.  float4 columns when d % 4 == 0, one float per
 * thread otherwise.  B, N, d <= 0 or a NULL pointer: TEMP_E_BADARG, nothing is launched.  (B = 1: a relation pair table.) */
int temp_pair_rows_fwd(int B, int N, int d, const float* a, const float* a_inv, float* out, void* stream);
int temp_pair_rows_bwd(int B, int N, int d, const float* d_out, float* d_a, float* d_a_inv, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Plain fp32 MFMA GEMMs (the extra (n,D)@(D,D) terms of the linear-recurrence layers,
 * models/RRGCN.py:141, models/BiRRGCN.py:128-129; the all-entity score matrix below).
 *   temp_linear    C[M,N] = A[M,K] . B          B is [K,N] (trans_b = 0) or stored as [N,K] (trans_b = 1)
 *   temp_linear_tn out[Ka,Nb] = A[M,Ka]^T . B[M,Nb]      (deterministic split over M)
 * K, N, Ka, Nb and all leading dimensions must be multiples of 4.
 * ---------------------------------------------------------------------------------------------- */
int temp_linear(int M, int N, int K, const float* A, int lda, const float* B, int ldb, int trans_b, float* C, int ldc, void* stream);
/* Same product, result stored TRANSPOSED: Ct[N, ldct] with Ct[n, m] = (A . B)[m, n]  (ldct >= M).  For "few rows x many columns"
 * outputs -- a window's ~200 positives scored against 10 000 entities -- the entity axis is made the tall one:
 * scores[P, N_ents] = temp_linear_t(M = N_ents, N = P, A = all_embeds, B = queries (trans_b = 1), Ct = scores). */
int temp_linear_t(int M, int N, int K, const float* A, int lda, const float* B, int ldb, int trans_b, float* Ct, int ldct, void* stream);
/* Several independent products of the same shape class in ONE launch sequence (up to 4 problems per launch):
 *   C_i[M_i, N] = A_i[M_i, K] . B_i        same N, K, leading dimensions and transposition; M_i may differ.
 * The per-window score matrices of the loss (every window scores against its own all-entity table) and their
 * input gradients.  `probs` is a HOST array. */
typedef struct TempLinearProblem { int M; const float* A; const float* B; float* C; } TempLinearProblem;
int temp_linear_multi(int count, const TempLinearProblem* probs, int N, int K, int lda, int ldb, int trans_b, int ldc, void* stream);
size_t temp_linear_tn_workspace(int M, int Ka, int Nb);
int temp_linear_tn(int M, int Ka, int Nb, const float* A, int lda, const float* B, int ldb, float* out, int ldo,
                   void* workspace, size_t workspace_bytes, void* stream);
/* Several weight-gradient-shaped products in one launch sequence (the per-window d_all_b = d_scores_b^T . q_b of the loss,
 * models/TKG_Module.py:202-213 differentiated): C_i[Ka,Nb] = A_i[M_i,Ka]^T . B_i[M_i,Nb], same Ka, Nb and leading dimensions,
 * C_i contiguous (ldc == Nb).  Small M_i run as ONE launch (up to 8 problems, problem index in the grid); shapes of the large-M
 * kernels fall back to one temp_linear_tn per problem.  `probs` is a HOST array; deterministic. */
size_t temp_linear_tn_multi_workspace(int count, int max_m, int Ka, int Nb);
int temp_linear_tn_multi(int count, const TempLinearProblem* probs, int Ka, int Nb, int lda, int ldb, int ldc, void* workspace,
                         size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Link-prediction loss (TKG_Module.train_link_prediction, models/TKG_Module.py:202-213;
 * utils/scores.py:4-44).  DistMult and ComplEx are bilinear in (query, candidate), so the scores of
 * the P positives against ALL N entities are ONE GEMM  scores = query[P,D] . all_embeds[N,D]^T
 * (temp_linear, trans_b = 1); the reference instead gathers a (P, 1+neg, D) tensor (1.2 GB at
 * P = 3000, neg = 500).  These two calls do the cross-entropy with label 0 over cand[P,C]
 * (column 0 = the true entity, global ids):
 *   fwd: loss_rows[p] = logsumexp_k scores[p, cand[p,k]] - scores[p, cand[p,0]];  lse_rows saved
 *   bwd: d_scores[P,N] (fully written) = scale[0] * inv_rows * sum_k (softmax_k - [k==0]) e_{cand[p,k]}
 *        (`scale` is a DEVICE float: the upstream gradient of the mean loss)
 * ---------------------------------------------------------------------------------------------- */
int temp_gather_ce_fwd(int P, int C, int N, const float* scores, const int32_t* cand, float* loss_rows, float* lse_rows, void* stream);
int temp_gather_ce_bwd(int P, int C, int N, const float* scores, const int32_t* cand, const float* lse_rows, const float* scale,
                       float inv_rows, const float* row_scale /* nullable [P]: per-row weight instead of inv_rows */, float* d_scores, void* stream);

/* ------------------------------------------------------------------------------------------------
 * All-entity ("1-vs-all") link-prediction loss: softmax cross-entropy of the true entity against EVERY entity outside the row's
 * known-true list -- the limit of temp_corrupt_sample + temp_gather_ce_* as negative_rate grows: each admissible entity exactly once,
 * no candidate matrix, no draws.  (No counterpart in the reference, which only samples.)
 * scores [P, ld] = P query rows scored against the N entities col0 .. col0 + N - 1 (column j < N is entity col0 + j; the producers of
 * temp_gather_ce_fwd).  The filter list of row p is ids[lo[p] .. hi[p]): GLOBAL entity ids, unique and ascending -- the arrays
 * temp_corrupt_sample takes, as they are (no CSR rebuild); lo == NULL (then hi == NULL): nothing is filtered.
 *   entity e is ADMISSIBLE for row p  <=>  e == truth[p]  or  e is not in the row's list
 * A filtered entity never enters the sum (it is excluded, not subtracted afterwards: the known-true entities are the ones with the
 * largest scores, and one of them may hold the row's maximum).
 *   fwd: an online softmax over the admissible columns of this panel.  carry = 0 starts the row state (run_max, run_sum,
 *        truth_score) [P each] fresh: (max, sum_j exp(s_j - max)) over the panel's admissible columns, (-inf, 0) when there is none,
 *        truth_score = scores[p, truth[p] - col0] when the truth lies in the panel, else 0.  carry = 1 merges into the state earlier
 *        calls left over DISJOINT entity ranges; a panel without an admissible column for a row leaves that row's state unchanged,
 *        bit for bit.  After every call  lse_rows = run_max + log(run_sum),  loss_rows = lse_rows - truth_score  (unscaled; meaningful
 *        once every panel has been seen; -inf, never NaN, while nothing admissible has).  Over panels the result equals ONE call over
 *        the union up to rounding.
 *   bwd: d_scores[p,j] = scale[0] * (row_scale ? row_scale[p] : inv_rows) * (exp(scores[p,j] - lse_rows[p]) - [col0 + j == truth[p]])
 *        for admissible columns, exactly 0 for filtered columns and for the pad columns N <= j < ld; a row whose factor is 0 is
 *        exactly 0.  d_scores [P, ld] is fully written.  `scale` is a DEVICE float, as in temp_gather_ce_bwd.
 * The row is STREAMED (float4 loads, 256 columns per wave and step), the list walked beside it 64 entries at a time in the wave's
 * registers: no LDS ceiling on N (temp_gather_ce_bwd refuses N > 40 704), any list length.  Dispatch, both calls: N <= 1024 one WAVE
 * per row, four rows per workgroup (no barrier); above that one 256-thread workgroup per row.
 * P >= 0, N > 0, ld >= N, col0 >= 0, col0 + ld + 256 < 2^31, carry in {0, 1} (else TEMP_E_BADARG); ld % 4 == 0 and scores (d_scores)
 * 16-byte aligned (else TEMP_E_UNSUPPORTED).  P == 0 succeeds without a launch.  No workspace, no floating-point atomics, one
 * reduction order per launch shape: bit-repeatable.  +inf and NaN scores are unspecified.
 * ---------------------------------------------------------------------------------------------- */
int temp_filtered_ce_fwd(int P, int N, int ld, int col0, const float* scores, const int32_t* truth, const int32_t* lo, const int32_t* hi,
                         const int32_t* ids, int carry, float* run_max, float* run_sum, float* truth_score, float* lse_rows, float* loss_rows,
                         void* stream);
int temp_filtered_ce_bwd(int P, int N, int ld, int col0, const float* scores, const int32_t* truth, const int32_t* lo, const int32_t* hi,
                         const int32_t* ids, const float* lse_rows, const float* scale, float inv_rows,
                         const float* row_scale /* nullable [P] */, float* d_scores, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Folded query of the scorers, row gathers fused in (utils/scores.py:4-12 distmult, :26-44 complex, :46-55 transE;
 * the s / r / o row selections of train_link_prediction, models/TKG_Module.py:202-213):
 *   k = ent_rows[known_idx[p]], r = rel[rel_idx[p]]          (both [*, d] row-major, d % 4 == 0; complex: d % 8 == 0)
 *   is_tail[p] != 0: k is the subject and candidates are objects (mode 'tail'), else k is the object and candidates are
 *   subjects (mode 'head'; ignored by distmult).
 *   distmult / complex: q[p] such that  score(p, candidate c) = <q[p], c>  (an inner-product query);
 *   transE:             q[p] = k + r (tail) or k - r (head), a translation query:  score(p, c) = -|q[p] - c|_1.  One IEEE
 *                       add / subtract per element, bit-equal to the tensor expression.
 *   simple (SimplE, utils/scores.py:14-24): the rows are PAIR rows of width d = 2 h, d % 8 == 0 -- k = [e | e_inv], r = [rel | rel_inv],
 *                       a candidate c = [o | o_inv] (temp_pair_rows_fwd builds such tables) -- and
 *                         q[p] = 1/2 [k[h:] r[h:] | k[:h] r[:h]]  (tail)      q[p] = 1/2 [k[h:] r[:h] | k[:h] r[h:]]  (head)
 *                       so that <q[p], c> = 1/2 (<s r, o_inv> + <s_inv r_inv, o>) resp. 1/2 (<s, r o_inv> + <s_inv, r_inv o>): an
 *                       inner-product query like distmult / complex.  The factor 1/2 is exact: every element of q and of the
 *                       gradients is one rounded product.  is_tail is required.  temp_gated_query_* do not take this kind.
 *   bwd: per-row gradients d_known_rows[p], d_rel_rows[p] (the caller sums them over the index lists); transE: d_q and +-d_q.
 * ---------------------------------------------------------------------------------------------- */
#define TEMP_SCORE_DISTMULT 0
#define TEMP_SCORE_COMPLEX 1
#define TEMP_SCORE_TRANSE 2
#define TEMP_SCORE_SIMPLE 3
int temp_bilinear_query_fwd(int P, int d, int kind, const float* ent_rows, const int32_t* known_idx, const float* rel, const int32_t* rel_idx,
                            const int32_t* is_tail, float* q, void* stream);
int temp_bilinear_query_bwd(int P, int d, int kind, const float* ent_rows, const int32_t* known_idx, const float* rel, const int32_t* rel_idx,
                            const int32_t* is_tail, const float* d_q, float* d_known_rows, float* d_rel_rows, void* stream);

/* ------------------------------------------------------------------------------------------------
 * TransE loss and scores (utils/scores.py:46-55 with the translation query q above):  score(p, c) = -sum_d |q[p,d] - c[d]|.
 * Not bilinear, so no GEMM: the loss reads the score at the C = 1 + negative_rate candidates of every row only (a gather of
 * P C d elements; the dense matrix is N / C times more), the ranking takes a dense VALU-tiled pass.
 *
 * temp_l1_ce_fwd: cross-entropy with label 0 over cand[P, C] (column 0 = the true entity):
 *   s_out[p,k] = -sum_d |q[p,d] - table[base[p] + cand[p,k], d]|     (base NULL = 0.  One launch covers all windows of a batch:
 *                table = the (B N, d) stack of the windows' all-entity matrices, base[p] = b N for a row of window b)
 *   lse_rows[p] = logsumexp_k s_out[p,k];   loss_rows[p] = lse_rows[p] - s_out[p,0].      C == 1: loss exactly 0.
 * temp_l1_ce_bwd_q:
 *   g_out[p,k] = scale[0] * (row_scale ? row_scale[p] : inv_rows) * (exp(s[p,k] - lse_rows[p]) - [k == 0])   (as temp_gather_ce_bwd)
 *   d_q[p,:]   = -sum_k g_out[p,k] sgn(q[p,:] - e_k),  sgn(0) = 0 (torch.abs's gradient), e_k the candidate's table row;
 *                duplicate candidates each count, a weight-0 row gives zeros.
 * temp_l1_ce_bwd_table: the candidate-side adjoint, without atomics:
 *   slot[P C] = the flat positions p C + k sorted by their table row base[p] + cand[p,k], ascending within a row (a stable sort);
 *   slot_ptr[n_rows + 1] = the CSR over table rows;
 *   d_table[n,:] = sum_{i in [slot_ptr[n], slot_ptr[n+1])} g[slot[i]] sgn(q[slot[i] / C, :] - table[n,:]);  zeros for a row without slots.
 * temp_l1_scores: scores[p,n] = -|q[p] - table[n]|_1 for n < N, -inf for N <= n < ld  ([P, ld]: feeds temp_filtered_rank directly).
 *
 * d % 4 == 0, P C < 2^31, ld % 4 == 0, else TEMP_E_UNSUPPORTED; P == 0 (n_rows == 0) returns success without a launch.  fp32,
 * all outputs fully written, no workspace, no floating-point atomics; every sum has a fixed order: results are bit-repeatable.
 * ---------------------------------------------------------------------------------------------- */
int temp_l1_ce_fwd(int P, int C, int d, const float* q, const float* table, const int32_t* base /* nullable [P] */, const int32_t* cand,
                   float* s_out, float* loss_rows, float* lse_rows, void* stream);
int temp_l1_ce_bwd_q(int P, int C, int d, const float* q, const float* table, const int32_t* base /* nullable [P] */, const int32_t* cand,
                     const float* s, const float* lse_rows, const float* scale /* device float */, float inv_rows,
                     const float* row_scale /* nullable [P] */, float* g_out, float* d_q, void* stream);
int temp_l1_ce_bwd_table(int n_rows, int d, int C, const float* q, const float* table, const int32_t* slot_ptr, const int32_t* slot,
                         const float* g, float* d_table, void* stream);
int temp_l1_scores(int P, int N, int d, const float* q, const float* table, int ld, float* scores, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Gated loss of the post-aggregation models (PostDynamicRGCN / PostBiDynamicRGCN.train_link_prediction,
 * models/PostDynamicRGCN.py:261-282): the known entity and the candidates are per-triple mixes w * local + (1 - w) * temporal
 * of the two embedding streams.  Both scorers are linear in the candidate, so the candidate mix is taken on the two score
 * matrices s_a = q . all_loc^T and s_b = q . all_rec^T (temp_linear_multi) at the candidate columns only.
 *
 * Gated folded query (the fold of temp_bilinear_query_fwd on a mixed known row; A, B, rel [*, d] row-major):
 *   known[p] = w[p] * A[ia[p]] + (1 - w[p]) * B[ib[p]]          when ia[p] >= 0
 *   known[p] = B[ib[p]]  (exactly; w[p] is not read)            when ia[p] <  0   -- TEMPORAL-ONLY row: the reference's head rows,
 *            whose "local" known object is the temporal row too (models/PostDynamicRGCN.py:276-277), so w[p] has no effect
 *   q[p]     = fold(known[p], rel[rel_idx[p]]) for kind / is_tail as in temp_bilinear_query_fwd; kind TEMP_SCORE_TRANSE gives the
 *              translation query known[p] + r (tail) / known[p] - r (head): one IEEE add / subtract after the mix (is_tail required).
 *   The mix is the one expression fmaf(w, a, (1 - w) * b) in every gated kernel, forward and backward (csrc/mix.hpp): for finite
 *   rows w == 1 gives a and w == 0 gives b bit-exactly.
 *   bwd (d_k = the gradient of known[p] from d_q[p]):
 *     d_a_rows[p] = w[p] d_k, d_b_rows[p] = (1 - w[p]) d_k, d_w[p] = <d_k, A[ia[p]] - B[ib[p]]>     (ia[p] >= 0)
 *     d_a_rows[p] = 0,        d_b_rows[p] = d_k,            d_w[p] = 0                            (ia[p] <  0)
 *     transE: d_k = d_q[p] and d_rel_rows[p] = +-d_q[p].
 *     d_rel_rows[p] = the relation row's gradient.  All outputs fully written ([P, d] and [P]); the caller sums the rows over the
 *     index lists (temp_segment_sum_rows; ia's negative entries are left out of its segmentation).
 *   d % 4 == 0 (complex: d % 8 == 0), else TEMP_E_UNSUPPORTED.  One wave per row; d_w is a wave reduction in fixed order.
 *
 * Gated candidate cross-entropy (label 0 over cand[P, C], column 0 = the true entity, entries in [0, N)):
 *   m[p, e] = w[p] * s_a[p, e] + (1 - w[p]) * s_b[p, e]   (s_a, s_b [P, N]; formed at the candidate columns only)
 *   fwd: loss_rows[p] = logsumexp_k m[p, cand[p,k]] - m[p, cand[p,0]];  lse_rows saved
 *   bwd: G[p, e] = scale[0] * (row_scale ? row_scale[p] : inv_rows) * sum_k (softmax_k - [k == 0]) [cand[p,k] == e]
 *        (duplicate candidates accumulate, as in temp_gather_ce_bwd);  d_s_a = w G, d_s_b = (1 - w) G  ([P, N] each, fully written,
 *        zero off-candidate);  d_w[p] = sum_e G[p, e] (s_a - s_b)[p, e].  N * 4 bytes must fit the LDS (N <= 40704), else
 *        TEMP_E_UNSUPPORTED.
 * fp32; no floating-point atomics (candidate multiplicities are integer LDS counters) and no workspace: results are bit-repeatable.
 * ---------------------------------------------------------------------------------------------- */
int temp_gated_query_fwd(int P, int d, int kind, const float* A, const int32_t* ia, const float* B, const int32_t* ib, const float* w,
                         const float* rel, const int32_t* rel_idx, const int32_t* is_tail, float* q, void* stream);
int temp_gated_query_bwd(int P, int d, int kind, const float* A, const int32_t* ia, const float* B, const int32_t* ib, const float* w,
                         const float* rel, const int32_t* rel_idx, const int32_t* is_tail, const float* d_q, float* d_a_rows, float* d_b_rows,
                         float* d_rel_rows, float* d_w, void* stream);
int temp_gather_ce_mix_fwd(int P, int C, int N, const float* s_a, const float* s_b, const float* w, const int32_t* cand, float* loss_rows,
                           float* lse_rows, void* stream);
int temp_gather_ce_mix_bwd(int P, int C, int N, const float* s_a, const float* s_b, const float* w, const int32_t* cand, const float* lse_rows,
                           const float* scale, float inv_rows, const float* row_scale /* nullable [P] */, float* d_s_a, float* d_s_b,
                           float* d_w, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Frozen-ensemble candidate cross-entropy (Aggregator, models/aggregator.py:200-206, 339-342): two FROZEN streams score the same
 * candidate lists from their own tables, possibly of different widths, and a per-row weight mixes the scores.  cand [P, C] int32,
 * column 0 = the true entity, holds ROW indices of both tables (the (B N_ents, D) stacks of the windows' all-entity matrices, the
 * window offset already added); row offsets are formed in 64 bits.
 *   kind TEMP_FROZEN_DOT: a_c = <q_a[p], T_a[cand[p,c]]>      (the folded bilinear query of temp_bilinear_query_fwd: distmult, complex)
 *   kind TEMP_FROZEN_L1:  a_c = -|q_a[p] - T_a[cand[p,c]]|_1  (the translation query: transE)
 *   b_c the same on (q_b, T_b);   x_c = mix(w[p], a_c, b_c) = fmaf(w, a_c, (1 - w) * b_c)   (csrc/mix.hpp: w == 1 gives a_c, w == 0 b_c)
 *   loss_rows[p] = logsumexp_c x_c - x_0                                                      (unscaled, as temp_gather_ce_mix_fwd)
 *   d_w[p]       = (row_scale ? row_scale[p] : inv_rows) * (sum_c softmax_c (a_c - b_c) - (a_0 - b_0))
 * A candidate listed twice counts twice.  Nothing else has a gradient, so there is no backward call and nothing is saved.  ONE launch
 * (one wave per row; an online logsumexp per group of 16 lanes, merged in a fixed order), no (P, N) score matrix, no workspace, no
 * atomics: results are bit-repeatable.  C == 1: the loss and d_w are exactly 0.
 * Da, Db: multiples of 4 in [4, 512], else TEMP_E_UNSUPPORTED before any launch (outputs untouched).  P == 0 succeeds without a launch;
 * P < 0, C <= 0, an unknown kind, or a NULL pointer (row_scale excepted) with P > 0: TEMP_E_BADARG.
 * ---------------------------------------------------------------------------------------------- */
#define TEMP_FROZEN_DOT 0
#define TEMP_FROZEN_L1 1
int temp_frozen_mix_ce(int P, int C, int Da, int Db, int kind, const float* q_a, const float* T_a, const float* q_b, const float* T_b,
                       const float* w, const int32_t* cand, const float* row_scale /* nullable [P] */, float inv_rows, float* loss_rows,
                       float* d_w, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Gated TransE loss and scores of the post-aggregation models (models/PostDynamicRGCN.py:261-282, utils/post_evaluation.py:32-69 with
 * utils/scores.py:46-55).  The candidate of row p is the mix of the two all-entity tables with the row's candidate weight,
 *   e[p,k] = mix(w[p], table_a[base[p] + cand[p,k]], table_b[base[p] + cand[p,k]]),    mix(w, a, b) = fmaf(w, a, (1 - w) * b),
 * and |q - e|_1 is not linear in e, so the mix cannot be taken on two score matrices as for the bilinear scorers: these are the
 * temp_l1_* calls above reading both table rows of a candidate and mixing in registers (table_a, table_b: the same shape, e.g. the
 * (B N, d) stacks of the windows' local and temporal all-entity matrices; q from temp_gated_query_fwd, kind TEMP_SCORE_TRANSE).
 *
 * temp_l1_mix_ce_fwd:   s_out[p,k] = -sum_d |q[p,d] - e[p,k,d]|;  lse_rows, loss_rows as temp_l1_ce_fwd (C == 1: loss exactly 0).
 * temp_l1_mix_ce_bwd_q: g_out as temp_l1_ce_bwd_q;  d_q[p,:] = -sum_k g_out[p,k] sgn(q[p,:] - e[p,k,:])  (sgn(0) = 0);
 *                       d_w[p] = sum_k g_out[p,k] sum_d sgn(q[p,d] - e[p,k,d]) (table_a - table_b)[row, d]     ([P], same pass).
 * temp_l1_mix_ce_bwd_table (slot lists as temp_l1_ce_bwd_table, over the shared row index of both tables):
 *   d_table_a[n,:] = sum_slots w[p] g[slot] sgn(q[p,:] - e),  d_table_b[n,:] = sum_slots (1 - w[p]) g[slot] sgn(q[p,:] - e),  p = slot / C;
 *   one pass over the row's slots writes both; zeros for a row without slots.
 * temp_l1_mix_scores:   scores[p,n] = -|q[p] - mix(w[p], table_a[n], table_b[n])|_1 for n < N, -inf for N <= n < ld (feeds
 *                       temp_filtered_rank: the ranking pass of PostEvaluationFilter).
 *
 * The contract of the temp_l1_* calls: d % 4 == 0, P C < 2^31, ld % 4 == 0, else TEMP_E_UNSUPPORTED; P == 0 (n_rows == 0) returns
 * success without a launch.  fp32, all outputs fully written, no workspace, no floating-point atomics; every sum has a fixed
 * order: results are bit-repeatable.
 * ---------------------------------------------------------------------------------------------- */
int temp_l1_mix_ce_fwd(int P, int C, int d, const float* q, const float* table_a, const float* table_b, const float* w,
                       const int32_t* base /* nullable [P] */, const int32_t* cand, float* s_out, float* loss_rows, float* lse_rows, void* stream);
int temp_l1_mix_ce_bwd_q(int P, int C, int d, const float* q, const float* table_a, const float* table_b, const float* w,
                         const int32_t* base /* nullable [P] */, const int32_t* cand, const float* s, const float* lse_rows,
                         const float* scale /* device float */, float inv_rows, const float* row_scale /* nullable [P] */, float* g_out,
                         float* d_q, float* d_w, void* stream);
int temp_l1_mix_ce_bwd_table(int n_rows, int d, int C, const float* q, const float* table_a, const float* table_b, const float* w,
                             const int32_t* slot_ptr, const int32_t* slot, const float* g, float* d_table_a, float* d_table_b, void* stream);
int temp_l1_mix_scores(int P, int N, int d, const float* q, const float* table_a, const float* table_b, const float* w, int ld,
                       float* scores, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Candidate-gather loss of the bilinear scorers (distmult / complex / simple with the inner-product query q of temp_bilinear_query_fwd
 * or temp_gated_query_fwd):  score(p, c) = +sum_d q[p,d] c[d], read at the C = 1 + negative_rate candidates of every row straight
 * from the table(s) -- the temp_l1_* calls above with a dot product where the L1 distance stands, argument for argument.  No (P, N)
 * score matrix and no LDS ceiling on the entity count (temp_gather_ce_bwd / temp_gather_ce_mix_bwd refuse N > 40704).
 *
 * temp_dot_ce_fwd:       s_out[p,k] = sum_d q[p,d] table[base[p] + cand[p,k], d]   (base NULL = 0; one launch covers all windows, as
 *                        temp_l1_ce_fwd);  lse_rows[p] = logsumexp_k s_out[p,k];  loss_rows[p] = lse_rows[p] - s_out[p,0].
 *                        C == 1: loss exactly 0.
 * temp_dot_ce_bwd_q:     g_out[p,k] = scale[0] * (row_scale ? row_scale[p] : inv_rows) * (exp(s[p,k] - lse_rows[p]) - [k == 0]);
 *                        d_q[p,:] = sum_k g_out[p,k] e_k,  e_k the candidate's table row.  Duplicate candidates each count; a
 *                        weight-0 row gives exact zeros in g_out and d_q (finite tables).
 * temp_dot_ce_bwd_table: slot / slot_ptr as temp_l1_ce_bwd_table;
 *                        d_table[n,:] = sum_{i in [slot_ptr[n], slot_ptr[n+1])} g[slot[i]] q[slot[i] / C, :];  zeros for a row without
 *                        slots.  `table` is checked but not read.
 * Gated (two tables, the row's candidate weight):  e[p,k] = mix(w[p], table_a[row], table_b[row]),  mix(w, a, b) = fmaf(w, a, (1 - w) * b),
 * formed in registers from both rows (w == 1 / w == 0 give the one-table scores of table_a / table_b):
 * temp_dot_mix_ce_fwd:       s_out[p,k] = sum_d q[p,d] e[p,k,d];  lse_rows, loss_rows as above.
 * temp_dot_mix_ce_bwd_q:     g_out as above;  d_q[p,:] = sum_k g_out[p,k] e[p,k,:];
 *                            d_w[p] = sum_k g_out[p,k] sum_d q[p,d] (table_a - table_b)[row, d]     ([P], same pass).
 * temp_dot_mix_ce_bwd_table: d_table_a[n,:] = sum_slots w[p] g[slot] q[p,:],  d_table_b[n,:] = sum_slots (1 - w[p]) g[slot] q[p,:],
 *                            p = slot / C;  one pass over the row's slots writes both; zeros for a row without slots.
 *
 * P < 0 (n_rows < 0), C <= 0, d <= 0: TEMP_E_BADARG;  d % 4 != 0 or P C >= 2^31: TEMP_E_UNSUPPORTED;  P == 0 (n_rows == 0) returns
 * success without a launch, before the pointer checks; with work, a NULL pointer where one is required is TEMP_E_BADARG (base and
 * row_scale are nullable; q, w, slot and g of a bwd_table call whose lists are all empty are not read).  fp32, all outputs fully
 * written, no workspace, no floating-point atomics; every sum has a fixed order: results are bit-repeatable.
 * ---------------------------------------------------------------------------------------------- */
int temp_dot_ce_fwd(int P, int C, int d, const float* q, const float* table, const int32_t* base /* nullable [P] */, const int32_t* cand,
                    float* s_out, float* loss_rows, float* lse_rows, void* stream);
int temp_dot_ce_bwd_q(int P, int C, int d, const float* q, const float* table, const int32_t* base /* nullable [P] */, const int32_t* cand,
                      const float* s, const float* lse_rows, const float* scale /* device float */, float inv_rows,
                      const float* row_scale /* nullable [P] */, float* g_out, float* d_q, void* stream);
int temp_dot_ce_bwd_table(int n_rows, int d, int C, const float* q, const float* table, const int32_t* slot_ptr, const int32_t* slot,
                          const float* g, float* d_table, void* stream);
int temp_dot_mix_ce_fwd(int P, int C, int d, const float* q, const float* table_a, const float* table_b, const float* w,
                        const int32_t* base /* nullable [P] */, const int32_t* cand, float* s_out, float* loss_rows, float* lse_rows, void* stream);
int temp_dot_mix_ce_bwd_q(int P, int C, int d, const float* q, const float* table_a, const float* table_b, const float* w,
                          const int32_t* base /* nullable [P] */, const int32_t* cand, const float* s, const float* lse_rows,
                          const float* scale /* device float */, float inv_rows, const float* row_scale /* nullable [P] */, float* g_out,
                          float* d_q, float* d_w, void* stream);
int temp_dot_mix_ce_bwd_table(int n_rows, int d, int C, const float* q, const float* table_a, const float* table_b, const float* w,
                              const int32_t* slot_ptr, const int32_t* slot, const float* g, float* d_table_a, float* d_table_b, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Snapshot store (build_interpolation_graphs / get_train_val_test_graph_at_t keep one DGL graph per timestamp,
 * utils/dataset.py:151-232,268-305; dgl.batch rebuilds the union every call, models/DynamicRGCN.py:92).  Here every
 * snapshot's sorted / chunked edge views stay resident on the device; a batch's TempGraph arrays are assembled from them
 * by ONE launch: descriptor j copies member array src[0..len) to out[dst_off ..) shifted by `add`
 *   mode 0: v + add     mode 1: v >= 0 ? v + add : v     mode 2: t = table[add + aux[i]]; t >= 0 ? t + v : t
 * and piece p = elements [piece_start[p], piece_start[p] + TEMP_ASSEMBLE_PIECE) of descriptor piece_desc[p].
 * All pointers are DEVICE pointers (descs included).
 * ---------------------------------------------------------------------------------------------- */
#define TEMP_ASSEMBLE_PIECE 4096
typedef struct TempCopyDesc { const int32_t* src; const int32_t* aux; int32_t dst_off; int32_t len; int32_t add; int32_t mode; } TempCopyDesc;
int temp_assemble_views(int n_pieces, const int32_t* piece_desc, const int32_t* piece_start, const TempCopyDesc* descs, const int32_t* table,
                        int32_t* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Device-side edge subsample of a resident snapshot: the training-time 50 % (target) / 80 %
 * (--random-dropout history) random edge subset with recomputed norms of DynamicRGCN.get_batch_graph_embeds
 * (models/DynamicRGCN.py:76-90; comp_deg_norm utils/utils.py:74-79), derived from the snapshot's resident sorted / chunked
 * views without a host rebuild or an upload.
 *   parent / child : packed view buffers of one snapshot with the layout of Snapshot.device_views (temp_amd/snapshot.py);
 *                    `child` must start as a copy of `parent`.  The call rewrites, in `child`, the a / b arrays of the three
 *                    views (kept edges moved to the front of every chunk, order preserved), their chunk_end arrays,
 *                    in_deg, out_deg and nnorm (1 / in_deg, 0 for isolated nodes); chunk tables, partial slots and fix-up
 *                    lists stay valid, so every temp_rgcn_* entry point runs on the child unchanged.
 *   eid [3][E]     : original edge id of every position of the by-dst / by-src / by-rel view.
 *   keep           : size of the subset; it is the set of the `keep` smallest values of a 64-bit counter hash of
 *                    (seed, edge id) -- a uniformly random `keep`-subset that depends on the seed only.
 *   keep_mask      : nullable [E] uint8 out, 1 = edge kept (original edge order).
 *   scratch        : >= 8 bytes of device memory per job.
 * `jobs` is a HOST array; all jobs of a batch run in three launches.
 * ---------------------------------------------------------------------------------------------- */
typedef struct TempSubsampleJob {
  int32_t n_nodes, n_edges, keep;
  uint64_t seed;
  const int32_t* parent; int32_t* child; const int32_t* eid;
  int32_t off_a[3], off_b[3], off_chunk_beg[3], off_chunk_end[3], off_chunk_seg[3], n_chunks[3];   /* word offsets inside a pack */
  int32_t off_in_deg, off_out_deg, off_nnorm;
  uint8_t* keep_mask; void* scratch;
} TempSubsampleJob;
int temp_subsample_views(int n_jobs, const TempSubsampleJob* jobs, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Filtered negative sampling (CorruptTriples.negative_sampling / corrupt_triple, utils/CorrptTriples.py:36-85):
 *   cand[row, 0] = truth[row];   cand[row, 1..K] = uniform draws over [0, N) that are not in the row's
 *   known-true set ids[lo[row] .. hi[row])  (global entity ids, ascending within a row; lo/hi NULL = no filter).
 * Exactly uniform over the entities outside the set: short sets by drawing the u-th entity of the complement directly,
 * long sets by rejection (binary search per attempt) with that as the fallback -- no unbounded resampling loop.
 * The draws are a counter-based hash of (seed, row, column, attempt): same seed => same samples, any launch shape.
 * cand: [R, 1+K] int32, fully written.
 * ---------------------------------------------------------------------------------------------- */
int temp_corrupt_sample(int R, int K, int N, uint64_t seed, const int32_t* truth, const int32_t* lo, const int32_t* hi, const int32_t* ids,
                        int32_t* cand, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Filtered ranking (EvaluationFilter.calc_metrics_single_graph / perturb_and_get_rank / sort_and_rank,
 * utils/evaluation.py:40-106).  scores [P, ld] = the P test triples scored against ALL N entities
 * (temp_linear with the folded query, trans_b = 1; temp_l1_scores for transE).  The reference overwrites the scores of the other
 * entities known to be true for the same (relation, known entity) with -10e6, applies a sigmoid and takes
 * the index of the target in a descending torch.sort.  Here:
 *   ranks[p] = 1 + #{ j : v_j > v_t  or  (v_j == v_t and j < target[p]) },
 *   v_j = sigmoid(scores[p,j]),  or 0 for j in the row's filter list  filt_ids[filt_ptr[p] .. filt_ptr[p+1])
 * (unique global ids; an entry equal to target[p] is ignored) -- the position in a STABLE descending order,
 * so exact sigmoid ties resolve by entity id where the reference's unstable sort leaves them arbitrary.
 * (TransE scores are negative L1 distances: below about -104 the fp32 sigmoid underflows to 0, as in the reference, and those
 * entities tie -- by entity id here.)
 * filt_ptr may be NULL (raw ranking); filt_ids may be NULL only when every list is empty.  ld % 4 == 0, ld >= N.  Integer output, deterministic.
 * ---------------------------------------------------------------------------------------------- */
int temp_filtered_rank(int P, int N, int ld, const float* scores, const int32_t* target, const int32_t* filt_ptr,
                       const int32_t* filt_ids, int32_t* ranks, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Streamed filtered ranking: temp_filtered_rank on a COLUMN PANEL of the score rows, with a carry, so that the [P, N] matrix of an
 * evaluation never has to exist at once; the _mix form ranks the mixed row of the two-table post models without writing it.
 * scores [P, ld] = the P rows scored against the entities col0 .. col0 + N - 1: column j < N is entity e = col0 + j.  target and
 * filt_ids hold GLOBAL entity ids; filt_ptr [P+1] / filt_ids as EvaluationFilter.filter_lists makes them (unique and ascending
 * within a row), nullable as for temp_filtered_rank.
 *   value of e:  0 for a listed entity that is not the row's target -- it is NOT excluded, and is ahead of a target whose own
 *                value is 0 when its id is smaller (TransE below about -104);  else v = sigmoid(x), temp_filtered_rank's own,
 *                x = scores[p,j]  (plain)   or   fmaf(w[p], a[p,j], (1 - w[p]) * b[p,j])  (mix: csrc/mix.hpp, in registers)
 *   e is AHEAD of the target  <=>  v > ts  or  (v == ts and e < target[p]);  the target itself is never ahead (its column goes
 *                through the same expressions as ts)
 *   columns j >= N are not entities and never count, whatever they hold (garbage, +inf): they are left out by index.
 * Operands at j < N are finite; +-inf and NaN there are OUTSIDE the contract (the mix of an infinity by a weight of 0 is NaN).
 * mode:
 *   TEMP_RANK_WHOLE        the panel holds every row's target: ts from the row itself, ranks[p] = 1 + #ahead.  target_score and count
 *                          may be NULL; only ranks is written.  The plain form returns temp_filtered_rank's ranks exactly.
 *   TEMP_RANK_COLLECT      rows whose target lies in [col0, col0 + N) write the raw (mixed) score of the target's column to
 *                          target_score[p]; other rows are not touched; nothing is counted (ranks and count may be NULL).
 *   TEMP_RANK_COUNT_FIRST  ts = sigmoid(target_score[p]);  count[p] = the panel's #ahead;  ranks[p] = count[p] + 1.
 *   TEMP_RANK_COUNT_ADD    the same with count[p] += the panel's #ahead.
 * A COLLECT sweep over disjoint panels that cover all entities, then a COUNT_FIRST / COUNT_ADD sweep over the same panels in any
 * order, equals ONE TEMP_RANK_WHOLE call over the concatenated row exactly (an integer sum).  count and ranks are int32.
 * P >= 0, N > 0, ld >= N, col0 >= 0, col0 + ld + 256 < 2^31, a known mode (else TEMP_E_BADARG); a NULL scores (scores_a, scores_b,
 * w), target, or output of the mode with P > 0: TEMP_E_BADARG; ld % 4 == 0 and the score matrices 16-byte aligned (else
 * TEMP_E_UNSUPPORTED) -- a column slice of a wider matrix with the wide ld qualifies.  P == 0 succeeds without a launch.  One wave
 * per row for N <= 1024, one workgroup per row above; no workspace, no atomics, bit-repeatable.
 * ---------------------------------------------------------------------------------------------- */
#define TEMP_RANK_WHOLE 0
#define TEMP_RANK_COLLECT 1
#define TEMP_RANK_COUNT_FIRST 2
#define TEMP_RANK_COUNT_ADD 3
int temp_filtered_rank_stream(int P, int N, int ld, int col0, const float* scores, const int32_t* target, const int32_t* filt_ptr,
                              const int32_t* filt_ids, int mode, float* target_score, int32_t* count, int32_t* ranks, void* stream);
int temp_filtered_rank_stream_mix(int P, int N, int ld, int col0, const float* scores_a, const float* scores_b, const float* w,
                                  const int32_t* target, const int32_t* filt_ptr, const int32_t* filt_ids, int mode, float* target_score,
                                  int32_t* count, int32_t* ranks, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Filtered top-k selection: the answer list of a query (s, r, ?, t) or (?, r, o, t), where temp_filtered_rank only locates one
 * known answer.  scores [P, ld] = P queries scored against the N entities col0 .. col0 + N - 1 (the same producers: temp_linear with
 * the folded query, temp_l1_scores); column j < N is the score of entity col0 + j, columns >= N never reach the result.
 *   entity e = col0 + j is ADMISSIBLE for row p  <=>  scores[p,j] > -inf  and  (e is not in the row's filter list
 *                                                     filt_ids[filt_ptr[p] .. filt_ptr[p+1])  or  e == keep[p])
 *   ORDER: higher score first, among equal scores the smaller entity id first -- total, the stable-descending convention of
 *          temp_filtered_rank, but on the RAW scores: the rank kernel's sigmoid saturates (every score above ~17 becomes 1.0f,
 *          every one below ~-104 becomes 0) and so manufactures ties, which is the reference's rank definition and useless for
 *          listing answers.  +inf is an ordinary score; NaN is unspecified.
 *   top_val / top_idx [P, k]: row p = the first min(k, #admissible) admissible entities in that order (score, global id), the
 *          remaining slots (-inf, -1).  Fully written.
 * carry = 0 starts fresh.  carry = 1 merges into the lists already in top_val / top_idx, which must be the result of earlier calls
 * over entity ranges disjoint from [col0, col0 + N): the result equals ONE call over the union of the ranges, bit for bit and in
 * any panel order (the selection is a function of the total order alone), so [P, N] never has to exist at once.
 * filt_ptr nullable [P+1] (NULL: nothing filtered); filt_ids = GLOBAL entity ids, unique and ascending within a row
 * (EvaluationFilter.filter_lists), NULL only when every list is empty; keep nullable [P], -1 = none.
 * 1 <= k <= TEMP_TOPK_MAX, N > 0, ld >= N, col0 >= 0 (else TEMP_E_BADARG); ld % 4 == 0 and scores 16-byte aligned (else
 * TEMP_E_UNSUPPORTED) -- a column slice base + c of a wider matrix, c % 4 == 0, with the wide ld qualifies.  P == 0 succeeds without a
 * launch.  No workspace, no floating-point atomics: bit-repeatable.
 * ---------------------------------------------------------------------------------------------- */
#define TEMP_TOPK_MAX 256
int temp_filtered_topk(int P, int N, int ld, int k, int col0, const float* scores, const int32_t* filt_ptr, const int32_t* filt_ids,
                       const int32_t* keep, int carry, float* top_val, int32_t* top_idx, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Filtered top-k selection over a MIXED score row: the answer list of a query on the two-table post models, which score against a
 * local and a temporal all-entity table and mix the two by a per-query gate.  The contract is temp_filtered_topk's, word for word,
 * on the row's mixed score
 *   m[p,j] = w[p] * a[p,j] + (1 - w[p]) * b[p,j],  evaluated as fmaf(w, a, (1 - w) * b) (csrc/mix.hpp: the one mixing expression of
 *            every gated kernel), formed in registers: the mixed matrix is neither written nor read.
 *   entity e = col0 + j is ADMISSIBLE for row p  <=>  a[p,j] > -inf  and  b[p,j] > -inf  and  (e is not in the row's filter list
 *                                                     or  e == keep[p])
 * The -inf test is made on the RAW operands, before the mix: w in {0, 1} would otherwise turn a -inf into 0 * inf = NaN or into a
 * finite score.  The pad columns of temp_l1_scores are -inf in both matrices and stay out.  Operands of +inf are OUTSIDE the
 * contract (fmaf(0, +inf, b) is NaN), unlike in temp_filtered_topk; NaN is unspecified.
 * scores_a, scores_b [P, ld] share ld; ld % 4 == 0 and both 16-byte aligned (else TEMP_E_UNSUPPORTED).  w [P] fp32, not
 * range-checked.  k, N, col0, carry and P == 0 are checked and behave as in temp_filtered_topk; NULL scores_a, scores_b or w with
 * P > 0 is TEMP_E_BADARG.  With w == 1 and finite b the mix returns a bit for bit (w == 0 and finite a: b), so carry = 1 merges
 * with lists of either entry point.  No workspace, no floating-point atomics: bit-repeatable.
 * ---------------------------------------------------------------------------------------------- */
int temp_filtered_topk_mix(int P, int N, int ld, int k, int col0, const float* scores_a, const float* scores_b, const float* w,
                           const int32_t* filt_ptr, const int32_t* filt_ids, const int32_t* keep, int carry, float* top_val,
                           int32_t* top_idx, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Clipped Adam: the reference trainer's optimizer step, Trainer(gradient_clip_val) -> clip_grad_norm_(parameters, max_norm)
 * (main.py:128-129, utils/args.py:26) followed by Adam(lr, weight_decay = 1e-4) (models/TKG_Module.py:154-160), as one
 * deterministic multi-tensor pass over a DEVICE table with one row per tensor that has a gradient:
 *   1. norm = sqrt(sum g^2) over every row                                    (temp_grad_norm_clip)
 *   2. r = max_norm / (norm + 1e-6);  coef = r if (r < 1 or r != r) else 1     (a NaN passes, as through torch's clamp)
 *   3. per element, in place and in fp32, with the row's scalars               (temp_adam_clip_step)
 *        g' = coef g + weight_decay p
 *        m += one_minus_beta1 (g' - m)
 *        v  = beta2 v + one_minus_beta2 g' g'
 *        p -= step_size m / (sqrt(v) inv_bias2_sqrt + eps)
 *      step_size = lr / (1 - beta1^t), inv_bias2_sqrt = 1 / sqrt(1 - beta2^t): the caller computes every scalar in double from its
 *      host-side step count t and rounds once.
 * Non-finite gradients get no special case: one inf element gives norm = inf and coef = 0 (that element becomes NaN, every other
 * one takes a decay-only step); one NaN element gives coef = NaN and NaN in every updated element.
 * A CHUNK is TEMP_ADAM_CHUNK consecutive elements of one tensor (its last chunk may be short) and is owned by one workgroup;
 * chunks are numbered through the table in row order: first_chunk[0] = 0, first_chunk[t + 1] = first_chunk[t] +
 * ceil(n[t] / TEMP_ADAM_CHUNK), n_chunks = the total.  The table lives in device memory; the library cannot check its contents:
 * the pointers must cover n elements each and the chunk numbering must be exact.  p / g / m / v need 4-byte alignment only; a row
 * whose four pointers are 16-byte aligned moves float4s.  Rows must not overlap each other.
 *
 * temp_grad_norm_clip: norm_coef[0] = (float) norm, norm_coef[1] = (float) coef, both from double.  Every chunk stores one
 * double sum of squares to the workspace (temp_grad_norm_workspace(n_chunks) bytes, 8-byte aligned) and one workgroup adds them:
 * accumulation in double from the lane up, every order fixed by the table, no atomics -- bit-repeatable.  Two launches (one when
 * n_chunks == 0: norm 0, coef 1).  g is read with the default cache policy: the update reads it again.
 * temp_adam_clip_step: one launch; norm_coef as written by temp_grad_norm_clip on the same stream, or NULL for coef = 1 (no
 * clipping).  n_chunks == 0 succeeds without a launch.
 * Negative counts, a NULL table with n_chunks > 0, a NULL norm_coef in temp_grad_norm_clip: TEMP_E_BADARG; a missing or short
 * workspace: TEMP_E_WORKSPACE; nothing is launched in either case.
 * Neither call allocates, copies or synchronises.
 * ---------------------------------------------------------------------------------------------- */
#define TEMP_ADAM_CHUNK 4096
typedef struct TempAdamTensor {
  float* p; const float* g; float* m; float* v;     /* parameter, gradient, exp_avg, exp_avg_sq: n floats each */
  int64_t n;
  float step_size, inv_bias2_sqrt, one_minus_beta1, beta2, one_minus_beta2, eps, weight_decay;
  int32_t first_chunk;
} TempAdamTensor;                                   /* 72 bytes */
size_t temp_grad_norm_workspace(int n_chunks);
int temp_grad_norm_clip(int n_tensors, int n_chunks, const TempAdamTensor* table, double max_norm, void* ws, size_t ws_bytes,
                        float* norm_coef, void* stream);
int temp_adam_clip_step(int n_tensors, int n_chunks, const TempAdamTensor* table, const float* norm_coef, void* stream);

/* ------------------------------------------------------------------------------------------------
 * History attention of the self-attention encoder (SARGCNLayer.calc_result + attention,
 * models/SARGCN.py:25-53; callers models/SARGCN.py:39-62, models/SelfAttentionRGCN.py:88-96).
 * The reference builds a dense (n, T, D) tensor [history ..., current] (zero rows + a -10e9 additive
 * mask where a node was inactive) and projects all of it; here K / V are projected once per distinct
 * (snapshot, node) row into a table and every query row lists its active history rows:
 *   idx[i, t] (t < T-1) = row of the history table or -1 (masked: softmax weight exactly 0)
 *   position T-1 is the row's own current K / V (kc, vc).
 *   s[i,h,t] = <q[i,h,:], K[t][h,:]> / sqrt(d_k) + decay[t];  p = softmax_t;  o[i,h,:] = sum_t p V[t][h,:]
 *   out[i, d * heads + h] = o[i,h,d]      (the reference's transpose after squeeze, SARGCN.py:37)
 * heads must be 8 (SARGCN.py:21), D % 8 == 0, D <= 512, T <= 64.
 * fwd saves score [n, heads, T] (raw s, -inf where masked) and lse [n, heads] for bwd.
 * bwd: d_q / d_kc / d_vc fully written; d_kh / d_vh either ACCUMULATED with atomics (zero them first; rows are
 * shared between query rows) or, given the inverse maps, written once per table row; d_decay [T] accumulated when non-NULL.
 * ---------------------------------------------------------------------------------------------- */
typedef struct TempAttn {
  int32_t n, D, heads, T;
  const float* q;  int32_t ldq;                     /* [n, D] query projections */
  const float* kh; const float* vh; int32_t ldh;    /* history table K / V rows */
  const float* kc; const float* vc; int32_t ldc;    /* current-position K / V, row i */
  const int32_t* idx;                               /* [n, T-1] */
  const float* decay;                               /* [T] additive score bias or NULL */
} TempAttn;
int temp_sa_attn_fwd(const TempAttn* p, float* out, float* score, float* lse, void* stream);
int temp_sa_attn_bwd(const TempAttn* p, const float* out, const float* score, const float* lse, const float* d_out,
                     float* d_q, int ld_dq, float* d_kh, float* d_vh, int ld_dh, float* d_kc, float* d_vc, int ld_dc,
                     float* d_decay, int n_table, const int32_t* inv_ptr, const int32_t* inv_ref, float* ds_ws, void* stream);
/* Deterministic form: inv_ptr [n_table+1] / inv_ref = idx grouped by history-table row (ref = i * (T-1) + t, the static
 * maps of a prepared batch) and ds_ws [n * heads * T] scratch.  Then d_kh / d_vh rows [0, n_table) are each written once
 * by a second pass over the table (no atomics, no zero-fill needed).  With inv_ptr = NULL the atomic form above is used. */

/* Split current row.  Where the current state of query row i is a SUM of two rows -- an entity row that no window changes and a
 * per-window time row (the all-entity pass of the post-aggregation attention models) -- the (q | k | v) projection, being linear,
 * is taken of the two small tables once, and the kernel forms
 *   (q | k | v)[i] = pa[ia[i]] + pb[ib[i]]          (3D floats per row; one fp32 addition per element)
 * itself instead of reading a materialised [n, 3D] buffer.  p->q / kc / vc are not read (may be NULL); everything else of
 * TempAttn, the shape limits, out / score / lse and the two backward forms are those of temp_sa_attn_fwd / _bwd, with which the
 * results are bit-equal when those are fed the fp32 sums.  ia / ib [n]: rows of pa / pb (repeats allowed, every entry in range);
 * lda, ldb >= 3D.  bwd writes d_qkv [n, ld_dqkv >= 3D] = the gradient of the SUMMED row (d_q | d_k | d_v), fully written; the
 * caller reduces it over ia and over ib (temp_segment_sum_rows) for d_pa and d_pb. */
typedef struct TempAttnSplit {
  const float* pa; const int32_t* ia; int32_t lda;
  const float* pb; const int32_t* ib; int32_t ldb;
} TempAttnSplit;
int temp_sa_attn_split_fwd(const TempAttn* p, const TempAttnSplit* s, float* out, float* score, float* lse, void* stream);
int temp_sa_attn_split_bwd(const TempAttn* p, const TempAttnSplit* s, const float* out, const float* score, const float* lse,
                           const float* d_out, float* d_qkv, int ld_dqkv, float* d_kh, float* d_vh, int ld_dh, float* d_decay,
                           int n_table, const int32_t* inv_ptr, const int32_t* inv_ref, float* ds_ws, void* stream);

/* Device-memory bandwidth probe used by bench.py to calibrate the achievable HBM peak
 * (float4 copy of `bytes` bytes, dst and src must not overlap). */
int temp_copy_probe(const void* src, void* dst, size_t bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Per-kernel timing for bench.py's roofline (not used by the product path).  Between begin and end
 * every kernel launch of this library is bracketed by HIP events on its launch stream.
 * temp_trace_end() synchronises the device, returns up to `capacity` (kernel id, milliseconds)
 * records in launch order and releases the events.  One trace at a time.
 * ---------------------------------------------------------------------------------------------- */
int temp_trace_begin(int capacity);
int temp_trace_end(int* kernel_ids /*host*/, float* ms /*host*/, int capacity, int* n_out /*host*/);
const char* temp_trace_kernel_name(int kernel_id);

#ifdef __cplusplus
}
#endif
#endif /* TEMP_AMD_H */
