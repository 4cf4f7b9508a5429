"""Shapes that pin every route and template width of the dense-product dispatcher (temp_amd/csrc/gemm_wres.hpp:
launch_gemm_panel_multi, the branches of temp_linear_multi) and of the fp32 weight-gradient kernel (gemm_kernels.hip: gemm_tn),
shared by tests/test_gpu_gemm_routes.py.  Pure data: no torch, no GPU.

A case names the entry point, the rows of every problem of the launch, K, N, the layout of B, whether the operands carry padded
leading dimensions, the options in force, whether the caller hands row keys over, which weight matrix every problem uses, and the
launches the library must then count: {(route, width): launches of ONE call}, read back from temp_gemm_route_launches.  The
expectations below are what the counter reported on an MI355X (they were first worked out from the planners; where the two
disagreed the library decided and the shape was moved so that the named route is still hit -- see RESULTS at the end).

RESULTS (MI355X): what every case launched and its largest error, as a fraction of sum |a||b|, on the wide data.  Largest per
route: bx 5.94e-07, bx_t 5.94e-07, bxp 5.61e-07, bxr 5.45e-07, hxp 5.56e-07, hxr 4.60e-07, panel 6.79e-07, tn_split 3.12e-07, tn_w7 2.62e-07, tn_w8 1.18e-07, wres 6.79e-07, wres_split 4.88e-07.
    linear-1-K4-N4-kn                                              panel<1>                 3.493e-08
    linear-1-K4-N4-nk                                              panel<1>                 3.493e-08
    linear-33-K44-N36-kn                                           panel<1>                 1.968e-07
    linear-33-K44-N36-nk                                           panel<1>                 1.968e-07
    linear-129-K84-N100-kn                                         panel<1>                 3.085e-07
    linear-129-K84-N100-nk                                         panel<1>                 3.085e-07
    linear-130-K200-N200-kn                                        panel<1>                 3.563e-07
    linear-130-K200-N200-nk                                        panel<1>                 3.563e-07
    linear-4000-K24-N1540-kn                                       panel<1> + panel<4>      4.358e-07
    linear-4000-K24-N1540-nk                                       panel<1> + panel<4>      4.358e-07
    linear-4000-K24-N1572-kn                                       panel<2> + panel<4>      4.615e-07
    linear-4000-K24-N1572-nk                                       panel<2> + panel<4>      4.615e-07
    linear-4000-K24-N1604-kn                                       panel<3> + panel<4>      4.455e-07
    linear-4000-K24-N1604-nk                                       panel<3> + panel<4>      4.455e-07
    linear-4000-K24-N740-kn                                        panel<2>                 4.822e-07
    linear-4000-K24-N740-nk                                        panel<2>                 4.822e-07
    linear-4000-K24-N772-kn                                        panel<1> + panel<2>      4.029e-07
    linear-4000-K24-N772-nk                                        panel<1> + panel<2>      4.029e-07
    linear-4100-K40-N1540-kn                                       panel<1> + panel<4>      5.213e-07
    linear-4100-K40-N1540-nk                                       panel<1> + panel<4>      5.213e-07
    linear-5000-K4-N8-kn                                           panel<1>                 1.809e-07
    linear-5000-K4-N8-nk                                           panel<1>                 1.809e-07
    linear-4100-K604-N200-kn                                       panel<1>                 5.311e-07
    linear-4100-K604-N200-nk                                       panel<1>                 5.311e-07
    linear-20000-K200-N200-kn-BF16X30-GEMM_STREAM1                 panel<1> + panel<2>      6.789e-07
    linear-20000-K200-N200-nk-BF16X30-GEMM_STREAM1                 panel<1> + panel<2>      6.789e-07
    multi-300_0_37_130-K84-N100-kn-B0123                           panel<1>                 3.584e-07
    multi-300_0_37_130-K84-N100-nk-B0123                           panel<1>                 3.584e-07
    multi-300_0_37_130-K84-N100-kn-B0000                           panel<1>                 3.584e-07
    multi-300_0_37_130-K84-N100-nk-B0000                           panel<1>                 3.584e-07
    linear-129-K84-N100-kn-pad                                     panel<1>                 3.085e-07
    linear-129-K84-N100-nk-pad                                     panel<1>                 3.085e-07
    linear-4000-K24-N1572-kn-pad                                   panel<2> + panel<4>      4.615e-07
    linear-4000-K24-N1572-nk-pad                                   panel<2> + panel<4>      4.615e-07
    linear_t-300-K8-N16-kn                                         panel<1>                 2.212e-07
    linear_t-300-K8-N16-nk                                         panel<1>                 2.212e-07
    linear_t-37-K44-N36-kn                                         panel<1>                 2.275e-07
    linear_t-37-K44-N36-nk                                         panel<1>                 2.275e-07
    linear-4097-K8-N4-kn                                           wres<1>                  2.047e-07
    linear-4097-K8-N4-nk                                           wres<1>                  2.047e-07
    linear-4128-K8-N4-kn                                           wres<1>                  1.705e-07
    linear-4097-K12-N32-kn                                         wres<1>                  2.684e-07
    linear-4097-K12-N32-nk                                         wres<1>                  2.684e-07
    linear-4128-K12-N32-nk                                         wres<1>                  2.695e-07
    linear-4097-K200-N200-kn                                       wres<1>                  5.866e-07
    linear-4097-K200-N200-nk                                       wres<1>                  5.866e-07
    linear-4128-K200-N200-kn                                       wres<1>                  5.476e-07
    linear-4097-K600-N200-kn                                       wres<1>                  5.301e-07
    linear-4097-K600-N200-nk                                       wres<1>                  5.301e-07
    linear-4128-K600-N200-nk                                       wres<1>                  5.685e-07
    linear-4097-K200-N64-kn                                        wres<2>                  4.485e-07
    linear-4097-K200-N64-nk                                        wres<2>                  4.485e-07
    linear-4128-K200-N64-kn                                        wres<2>                  4.870e-07
    linear-4097-K200-N128-kn                                       wres<2>                  4.545e-07
    linear-4097-K200-N128-nk                                       wres<2>                  4.545e-07
    linear-4128-K200-N128-nk                                       wres<2>                  5.293e-07
    linear-4097-K208-N128-kn                                       wres<2>                  5.709e-07
    linear-4097-K208-N128-nk                                       wres<2>                  5.709e-07
    linear-4128-K208-N128-kn                                       wres<2>                  4.725e-07
    linear-4097-K208-N96-kn                                        wres<1>                  4.473e-07
    linear-4097-K208-N96-nk                                        wres<1>                  4.473e-07
    linear-4128-K208-N96-nk                                        wres<1>                  4.869e-07
    linear-4097-K200-N600-kn                                       wres<2>                  5.845e-07
    linear-4097-K200-N600-nk                                       wres<2>                  5.845e-07
    linear-4128-K200-N600-kn                                       wres<2>                  5.502e-07
    linear-4097-K200-N96-kn                                        wres<3>                  4.426e-07
    linear-4097-K200-N96-nk                                        wres<3>                  4.426e-07
    linear-4128-K200-N96-nk                                        wres<3>                  4.519e-07
    linear-4097-K72-N340-kn                                        wres<3>                  5.354e-07
    linear-4097-K72-N340-nk                                        wres<3>                  5.354e-07
    linear-4128-K72-N340-kn                                        wres<3>                  4.792e-07
    linear-4097-K200-N200-kn-pad                                   wres<1>                  5.866e-07
    linear-4097-K200-N200-nk-pad                                   wres<1>                  5.866e-07
    linear-4128-K72-N340-kn-pad                                    wres<3>                  4.792e-07
    linear-4128-K72-N340-nk-pad                                    wres<3>                  4.792e-07
    linear-20000-K200-N200-kn-BF16X30                              wres<1>                  6.789e-07
    linear-20000-K200-N200-nk-BF16X30                              wres<1>                  6.789e-07
    linear-20000-K200-N600-kn-BF16X30                              wres<2>                  5.778e-07
    linear-20000-K200-N600-nk-BF16X30                              wres<2>                  5.778e-07
    multi-2100_2100_37-K200-N200-kn-B000                           wres<1>                  4.881e-07
    multi-2100_2100_37-K200-N200-nk-B000                           wres<1>                  4.881e-07
    multi-2100_2100_37-K200-N200-kn-B012                           wres_split<1>            4.881e-07
    multi-2100_2100_37-K200-N200-nk-B012                           wres_split<1>            4.881e-07
    multi-2100_2100_37-K200-N200-kn-B001                           wres<1>                  4.881e-07
    multi-2100_2100_37-K200-N200-nk-B001                           wres<1>                  4.881e-07
    multi-0_2100_2100-K200-N200-kn-B000                            wres<1>                  1.950e+29   (before the fix of k_gemm_wres)
    multi-0_2100_2100-K200-N200-nk-B000                            wres<1>                  4.508e+19   (before the fix of k_gemm_wres)
    multi-2100_0_2100-K200-N200-kn-B011                            wres<1>                  1.405e+00   (before the fix of k_gemm_wres)
    multi-2100_0_2100-K200-N200-nk-B011                            wres<1>                  1.405e+00   (before the fix of k_gemm_wres)
    linear-16400-K72-N8-kn-keys                                    hxr                      2.909e-07
    linear-16400-K208-N132-nk-keys                                 hxr                      3.321e-07
    linear-16400-K136-N328-kn-keys                                 hxr                      3.442e-07
    linear-16400-K200-N600-nk                                      hxr                      4.268e-07
    linear-16400-K200-N200-kn                                      bxr                      5.025e-07
    linear-16400-K200-N200-nk-pad                                  bxr                      5.025e-07
    linear-16400-K72-N8-nk-F16X20                                  bxr                      3.316e-07
    linear-16400-K136-N328-kn-F16X20                               bxr                      4.981e-07
    linear-16400-K208-N132-nk-pad-keys                             hxr                      3.321e-07
    linear-16400-K36-N72-nk-keys                                   hxp<1>                   3.979e-07
    linear-16400-K500-N200-kn-keys                                 hxp<1>                   3.207e-07
    linear-16400-K600-N200-nk-pad-keys                             hxp<1>                   3.917e-07
    linear-16400-K200-N200-kn-pad-F16X20-GEMM_RESIDENT0            bxp<1>                   5.025e-07
    linear-16400-K24-N8-kn-keys                                    hxp<1>                   3.329e-07
    linear-16400-K600-N8-nk-keys                                   hxp<1>                   3.978e-07
    linear-16400-K200-N8-kn-F16X20-GEMM_RESIDENT0                  bxp<1>                   3.848e-07
    linear-16400-K24-N36-nk-keys                                   hxp<1>                   3.413e-07
    linear-16400-K600-N36-kn-keys                                  hxp<1>                   3.626e-07
    linear-16400-K200-N36-nk-F16X20-GEMM_RESIDENT0                 bxp<1>                   4.347e-07
    linear-16400-K24-N100-kn-keys                                  hxp<1>                   3.910e-07
    linear-16400-K600-N100-nk-keys                                 hxp<1>                   3.871e-07
    linear-16400-K200-N100-kn-F16X20-GEMM_RESIDENT0                bxp<1>                   5.613e-07
    linear-16400-K24-N132-nk-keys                                  hxp<2>                   4.511e-07
    linear-16400-K600-N132-kn-keys                                 hxp<2>                   3.299e-07
    linear-16400-K200-N132-nk-F16X20-GEMM_RESIDENT0                bxp<2>                   4.111e-07
    linear-16400-K24-N200-kn-keys                                  hxp<1>                   4.055e-07
    linear-16400-K600-N200-nk-keys                                 hxp<1>                   3.917e-07
    linear-16400-K200-N200-kn-F16X20-GEMM_RESIDENT0                bxp<1>                   5.025e-07
    linear-16400-K24-N328-nk-keys                                  hxp<4>                   4.094e-07
    linear-16400-K600-N328-kn-keys                                 hxp<4>                   5.559e-07
    linear-16400-K200-N328-nk-F16X20-GEMM_RESIDENT0                bxp<4>                   5.055e-07
    linear-16400-K24-N600-kn-keys                                  hxp<7>                   4.349e-07
    linear-16400-K600-N600-nk-keys                                 hxp<7>                   3.982e-07
    linear-16400-K200-N600-kn-F16X20-GEMM_RESIDENT0                bxp<7>                   5.611e-07
    linear-16400-K24-N1000-nk-keys                                 hxp<4>                   4.470e-07
    linear-16400-K600-N1000-kn-keys                                hxp<4>                   4.194e-07
    linear-16400-K200-N1000-nk-F16X20-GEMM_RESIDENT0               bxp<4>                   5.336e-07
    linear-16400-K24-N36-kn-F16X20-GEMM_RESIDENT0                  bxp<1>                   3.694e-07
    linear-16400-K24-N200-nk-F16X20-GEMM_RESIDENT0                 bxp<1>                   3.950e-07
    linear-16400-K600-N36-nk-F16X20-GEMM_RESIDENT0                 bxp<1>                   4.362e-07
    linear-16400-K600-N200-kn-F16X20-GEMM_RESIDENT0                bxp<1>                   5.530e-07
    linear-16400-K200-N2560-kn-F16X20-GEMM_RESIDENT0               bx<5>                    5.302e-07
    linear-16400-K200-N2560-nk-F16X20-GEMM_RESIDENT0               bx_t<5>                  5.302e-07
    linear-16400-K600-N1000-kn-F16X20-GEMM_RESIDENT0               bx<4>                    5.293e-07
    linear-16400-K600-N1000-nk-pad-F16X20-GEMM_RESIDENT0           bx_t<4>                  5.293e-07
    multi-9000_0_7400-K200-N600-nk-B000                            hxr                      4.002e-07
    multi-9000_0_7400-K200-N200-kn-B000                            bxr                      5.447e-07
    multi-9000_0_7400-K600-N200-kn-B000                            hxp<1>                   3.390e-07
    multi-9000_0_7400-K200-N200-nk-F16X20-GEMM_RESIDENT0-B000      bxp<1>                   5.447e-07
    multi-9000_0_7400-K600-N1000-kn-F16X20-GEMM_RESIDENT0-B000     bx<4>                    5.478e-07
    multi-9000_0_7400-K600-N1000-nk-F16X20-GEMM_RESIDENT0-B000     bx_t<4>                  5.478e-07
    multi-9000_0_7400-K200-N600-nk-B012                            hxr                      4.604e-07
    multi-9000_0_7400-K200-N200-kn-B012                            bxr                      5.447e-07
    multi-9000_0_7400-K600-N200-kn-B012                            hxp<1>                   3.157e-07
    multi-9000_0_7400-K200-N200-nk-F16X20-GEMM_RESIDENT0-B012      bxp<1>                   5.447e-07
    multi-9000_0_7400-K600-N1000-kn-F16X20-GEMM_RESIDENT0-B012     bx<4>                    5.939e-07
    multi-9000_0_7400-K600-N1000-nk-F16X20-GEMM_RESIDENT0-B012     bx_t<4>                  5.939e-07
    tn-300-K200-N32-kn                                             tn_w7<1>                 9.584e-08
    tn-300-K200-N40-kn                                             tn_w7<2>                 1.175e-07
    tn-300-K200-N100-kn                                            tn_w7<4>                 1.124e-07
    tn-300-K200-N200-kn                                            tn_split<7>              1.116e-07
    tn-300-K200-N200-kn-TN_SPLIT0                                  tn_w7<7>                 1.116e-07
    tn-300-K200-N328-kn                                            tn_w7<7>                 1.071e-07
    tn-300-K256-N100-kn                                            tn_w8<4>                 1.050e-07
    tn-300-K256-N200-kn-TN_SPLIT0                                  tn_w8<7>                 1.177e-07
    tn-300-K600-N200-kn                                            tn_split<7>              1.489e-07
    tn-300-K600-N100-kn                                            tn_w7<4>                 1.168e-07
    tn-300-K200-N100-kn-pad                                        tn_w7<4>                 1.124e-07
    tn-2049-K600-N200-kn-pad                                       tn_split<7>              6.268e-08
    tn-0-K200-N200-kn                                              tn_split<7>              0.000e+00
    tn-0-K200-N100-kn                                              tn_w7<4>                 0.000e+00
    tn-1-K200-N200-kn                                              tn_split<7>              5.928e-08
    tn-1-K200-N100-kn                                              tn_w7<4>                 5.913e-08
    tn-15-K200-N200-kn                                             tn_split<7>              2.530e-07
    tn-15-K200-N100-kn                                             tn_w7<4>                 2.622e-07
    tn-17-K200-N200-kn                                             tn_split<7>              3.121e-07
    tn-17-K200-N100-kn                                             tn_w7<4>                 2.540e-07
    tn-2047-K200-N200-kn                                           tn_split<7>              6.872e-08
    tn-2047-K200-N100-kn                                           tn_w7<4>                 6.087e-08
    tn-2049-K200-N200-kn                                           tn_split<7>              6.491e-08
    tn-2049-K200-N100-kn                                           tn_w7<4>                 7.099e-08
"""
import collections

# include/temp_amd.h: TEMP_ROUTE_*
ROUTES = ("panel", "wres", "wres_split", "bxp", "bx", "bx_t", "hxp", "bxr", "hxr", "kslice", "linear_t", "tn_w7", "tn_w8", "tn_split")
ROUTE_ID = {name: i for i, name in enumerate(ROUTES)}
WIDTHS = 8

# include/temp_amd.h: TEMP_OPT_*
OPT = {"BF16X3": 0, "TN_SPLIT": 1, "GEMM_STREAM": 3, "GEMM_RESIDENT": 8, "F16X2": 9}

Case = collections.namedtuple("Case", "entry Ms K N trans_b pad opts keys bpat expect")
Case.id = property(lambda c: "%s-%s-K%d-N%d-%s%s%s%s%s" % (
    c.entry, "_".join(str(m) for m in c.Ms), c.K, c.N, "nk" if c.trans_b else "kn", "-pad" if c.pad else "",
    "".join("-%s%d" % kv for kv in sorted(c.opts.items())), "-keys" if c.keys else "",
    "-B" + "".join(str(i) for i in c.bpat) if len(c.Ms) > 1 else ""))


def case(entry, Ms, K, N, trans_b, expect, pad=False, opts=None, keys=False, bpat=None):
    Ms = [Ms] if isinstance(Ms, int) else list(Ms)
    return Case(entry, tuple(Ms), K, N, bool(trans_b), pad, dict(opts or {}), keys, tuple(bpat or [0] * len(Ms)), dict(expect))


def _both(entry, Ms, K, N, expect, **kw):
    return [case(entry, Ms, K, N, t, expect, **kw) for t in (False, True)]


# ---------------------------------------------------------------------------------------------------------------------
# fp32 row panels, k_gemm_panel<NT>: rows < 4096 (WRES_MIN_ROWS), or shapes wres_plan refuses, or TEMP_OPT_GEMM_STREAM.
# The column-block width: 4 tiles while (row blocks of 128) x ceil(tiles / 4) >= 384, else 2, else 1; whole groups go to the
# `full` launch, the 1..3 tiles left over to the `rem` launch.
# ---------------------------------------------------------------------------------------------------------------------
FP32_OFF = {"BF16X3": 0}
PANEL = (
    _both("linear", 1, 4, 4, {("panel", 1): 1})                                  # the smallest shape
    + _both("linear", 33, 44, 36, {("panel", 1): 1})                             # one 40-chunk of K plus 4, K % 8 == 4, two column tiles
    + _both("linear", 129, 84, 100, {("panel", 1): 1})
    + _both("linear", 130, 200, 200, {("panel", 1): 1})
    + _both("linear", 4000, 24, 1540, {("panel", 4): 1, ("panel", 1): 1})        # 49 tiles: 12 groups of four + one tile
    + _both("linear", 4000, 24, 1572, {("panel", 4): 1, ("panel", 2): 1})
    + _both("linear", 4000, 24, 1604, {("panel", 4): 1, ("panel", 3): 1})
    + _both("linear", 4000, 24, 740, {("panel", 2): 1})                          # 24 tiles: twelve pairs, no rem launch
    + _both("linear", 4000, 24, 772, {("panel", 2): 1, ("panel", 1): 1})
    # rows >= 4096 that wres_plan refuses
    + _both("linear", 4100, 40, 1540, {("panel", 4): 1, ("panel", 1): 1})        # 17 resident slices
    + _both("linear", 5000, 4, 8, {("panel", 1): 1})                             # K < 8
    + _both("linear", 4100, 604, 200, {("panel", 1): 1})                         # a one-tile slice of K = 640 padded does not fit 80 KB
    + _both("linear", 20000, 200, 200, {("panel", 2): 1, ("panel", 1): 1}, opts={"GEMM_STREAM": 1, "BF16X3": 0})
    # several problems per launch (blockIdx.z), an empty one among them
    + _both("multi", [300, 0, 37, 130], 84, 100, {("panel", 1): 1}, bpat=(0, 1, 2, 3))
    + _both("multi", [300, 0, 37, 130], 84, 100, {("panel", 1): 1}, bpat=(0, 0, 0, 0))
    # lda = K + 4, ldb = width + 8 (ldc = N + 4 everywhere)
    + _both("linear", 129, 84, 100, {("panel", 1): 1}, pad=True)
    + _both("linear", 4000, 24, 1572, {("panel", 4): 1, ("panel", 2): 1}, pad=True)
    # the transposed store (EpiPlainStoreT), ldct = M + 3
    + _both("linear_t", 300, 8, 16, {("panel", 1): 1})
    + _both("linear_t", 37, 44, 36, {("panel", 1): 1})
)
# N % 4 != 0 (n_valid ragged inside a quad) is refused by this route: TEMP_E_UNSUPPORTED, nothing launched, nothing written
LINEAR_T_REFUSED = (37, 44, 34)

# ---------------------------------------------------------------------------------------------------------------------
# fp32 weights-resident, k_gemm_wres<NTS>: 4096 <= rows < 16384 (or any rows >= 4096 with TEMP_OPT_MFMA_BF16X3 = 0).
# M = 4097: 129 row panels, 17 per XCD, so the last XCD's range holds 10; M = 4128: 129 full panels.
# ---------------------------------------------------------------------------------------------------------------------
_WRES_SHAPES = (
    (8, 4, 1), (12, 32, 1),               # K zero-padded to 40; K % 8 == 4
    (200, 200, 1),                        # seven one-tile slices: the ICEWS step shape
    (600, 200, 1),                        # K at the LDS limit of a one-tile slice
    (200, 64, 2), (200, 128, 2),          # one slice / two slices of two tiles
    (208, 128, 2),                        # K padded to 240: LDS admits only two tiles
    (208, 96, 1),                         # ... and for three tiles the planner's cost then prefers three one-tile slices
    (200, 600, 2),                        # 19 tiles = 10 slices, the last one overlaps and stores one tile
    (200, 96, 3),
    (72, 340, 3),                         # 11 tiles = 4 slices, the last one overlaps and stores two tiles
)
WRES = []
for _i, (_K, _N, _w) in enumerate(_WRES_SHAPES):
    WRES += _both("linear", 4097, _K, _N, {("wres", _w): 1})
    WRES.append(case("linear", 4128, _K, _N, _i % 2, {("wres", _w): 1}))
WRES += (
    _both("linear", 4097, 200, 200, {("wres", 1): 1}, pad=True)
    + _both("linear", 4128, 72, 340, {("wres", 3): 1}, pad=True)
    # bps capped by the block budget instead of the panel count: every wave walks several panels
    + _both("linear", 20000, 200, 200, {("wres", 1): 1}, opts=FP32_OFF)
    + _both("linear", 20000, 200, 600, {("wres", 2): 1}, opts=FP32_OFF)
    + _both("multi", [2100, 2100, 37], 200, 200, {("wres", 1): 1}, bpat=(0, 0, 0))           # staged once
    + _both("multi", [2100, 2100, 37], 200, 200, {("wres_split", 1): 1}, bpat=(0, 1, 2))
    + _both("multi", [2100, 2100, 37], 200, 200, {("wres", 1): 1}, bpat=(0, 0, 1))           # re-staged behind the barrier
    # an empty problem in front of / between problems that share B: the staging decision must compare with the B that was
    # STAGED, not with the skipped problem's
    + _both("multi", [0, 2100, 2100], 200, 200, {("wres", 1): 1}, bpat=(0, 0, 0))
    + _both("multi", [2100, 0, 2100], 200, 200, {("wres", 1): 1}, bpat=(0, 1, 1))
)
WRES = tuple(WRES)

# ---------------------------------------------------------------------------------------------------------------------
# split-operand kernels: rows >= 16384 (BX_MIN_ROWS).  M = 16400: the last 128-row tile holds 16 rows.
#   P0 default options, no keys     P1 default, row keys from temp_absmax_keys
#   P2 F16X2 = 0                    P3 F16X2 = 0, GEMM_RESIDENT = 0
# G (tiles per column group) at 129 row tiles: N = 8, 36, 100, 200 -> 1;  132 -> 2 (3 groups, the last shifted);  328 -> 4 (3 groups,
# shifted);  600 -> 7 (3 groups, shifted);  1000 -> 4 (8 groups);  2560 -> 5 (16 groups);  at 157 row tiles (M = 20000) N = 200 -> 3
# (3 groups, shifted).  G = 6 is produced by none of these row counts.
# ---------------------------------------------------------------------------------------------------------------------
P2 = {"F16X2": 0}
P3 = {"F16X2": 0, "GEMM_RESIDENT": 0}
_G = {8: 1, 36: 1, 100: 1, 132: 2, 200: 1, 328: 4, 600: 7, 1000: 4, 2560: 5}
SPLIT = [
    case("linear", 16400, 72, 8, 0, {("hxr", 0): 1}, keys=True),
    case("linear", 16400, 208, 132, 1, {("hxr", 0): 1}, keys=True),
    case("linear", 16400, 136, 328, 0, {("hxr", 0): 1}, keys=True),
    case("linear", 16400, 200, 600, 1, {("hxr", 0): 1}),
    case("linear", 16400, 200, 200, 0, {("bxr", 0): 1}),
    case("linear", 16400, 200, 200, 1, {("bxr", 0): 1}, pad=True),
    case("linear", 16400, 72, 8, 1, {("bxr", 0): 1}, opts=P2),
    case("linear", 16400, 136, 328, 0, {("bxr", 0): 1}, opts=P2),
    case("linear", 16400, 208, 132, 1, {("hxr", 0): 1}, keys=True, pad=True),
    case("linear", 16400, 36, 72, 1, {("hxp", 1): 1}, keys=True),                 # K % 8 == 4
    case("linear", 16400, 500, 200, 0, {("hxp", 1): 1}, keys=True),
    case("linear", 16400, 600, 200, 1, {("hxp", 1): 1}, keys=True, pad=True),
    case("linear", 16400, 200, 200, 0, {("bxp", 1): 1}, opts=P3, pad=True),
    case("linear", 20000, 600, 200, 0, {("hxp", 3): 1}),                          # the GRU d_x shape: K >= 400 takes its own key pass
    case("linear", 20000, 600, 200, 1, {("bxp", 3): 1}, opts=P3),
]
for _i, _N in enumerate((8, 36, 100, 132, 200, 328, 600, 1000)):
    SPLIT.append(case("linear", 16400, 24, _N, _i % 2, {("hxp", _G[_N]): 1}, keys=True))
    SPLIT.append(case("linear", 16400, 600, _N, 1 - _i % 2, {("hxp", _G[_N]): 1}, keys=True))
    SPLIT.append(case("linear", 16400, 200, _N, _i % 2, {("bxp", _G[_N]): 1}, opts=P3))
SPLIT += [
    case("linear", 16400, 24, 36, 0, {("bxp", 1): 1}, opts=P3),
    case("linear", 16400, 24, 200, 1, {("bxp", 1): 1}, opts=P3),
    case("linear", 16400, 600, 36, 1, {("bxp", 1): 1}, opts=P3),
    case("linear", 16400, 600, 200, 0, {("bxp", 1): 1}, opts=P3),
    # packed weights over 3 MB: the blocks split B themselves
    case("linear", 16400, 200, 2560, 0, {("bx", 5): 1}, opts=P3),
    case("linear", 16400, 200, 2560, 1, {("bx_t", 5): 1}, opts=P3),
    case("linear", 16400, 600, 1000, 0, {("bx", 4): 1}, opts=P3),
    case("linear", 16400, 600, 1000, 1, {("bx_t", 4): 1}, opts=P3, pad=True),
]
# one multi-problem launch per family with an empty problem in the middle: shared B, distinct B
for _bp in ((0, 0, 0), (0, 1, 2)):
    SPLIT += [
        case("multi", [9000, 0, 7400], 200, 600, 1, {("hxr", 0): 1}, bpat=_bp),
        case("multi", [9000, 0, 7400], 200, 200, 0, {("bxr", 0): 1}, bpat=_bp),
        case("multi", [9000, 0, 7400], 600, 200, 0, {("hxp", 1): 1}, bpat=_bp),
        case("multi", [9000, 0, 7400], 200, 200, 1, {("bxp", 1): 1}, opts=P3, bpat=_bp),
        case("multi", [9000, 0, 7400], 600, 1000, 0, {("bx", 4): 1}, opts=P3, bpat=_bp),
        case("multi", [9000, 0, 7400], 600, 1000, 1, {("bx_t", 4): 1}, opts=P3, bpat=_bp),
    ]
SPLIT = tuple(SPLIT)

# ---------------------------------------------------------------------------------------------------------------------
# fp32 weight gradient out[Ka, Nb] = A[M, Ka]^T . B[M, Nb], k_gemm_tn<NT, WPB, SPLIT>, M < 4096.  For a `tn` case K is Ka and N is
# Nb.  NT by column tiles: 1 -> 1, 2 -> 2, 3..4 -> 4, >= 5 -> 7;  WPB 7 or 8, whichever pads ceil(Ka / 32) less;  5..7 column tiles
# take the SPLIT = 2 kernel unless TEMP_OPT_TN_SPLIT = 0.  The slice length changes at M = 2048.
# ---------------------------------------------------------------------------------------------------------------------
TN_OFF = {"TN_SPLIT": 0}
TN = [
    case("tn", 300, 200, 32, 0, {("tn_w7", 1): 1}),
    case("tn", 300, 200, 40, 0, {("tn_w7", 2): 1}),
    case("tn", 300, 200, 100, 0, {("tn_w7", 4): 1}),
    case("tn", 300, 200, 200, 0, {("tn_split", 7): 1}),
    case("tn", 300, 200, 200, 0, {("tn_w7", 7): 1}, opts=TN_OFF),
    case("tn", 300, 200, 328, 0, {("tn_w7", 7): 1}),                              # two column blocks
    case("tn", 300, 256, 100, 0, {("tn_w8", 4): 1}),
    case("tn", 300, 256, 200, 0, {("tn_w8", 7): 1}, opts=TN_OFF),
    case("tn", 300, 600, 200, 0, {("tn_split", 7): 1}),
    case("tn", 300, 600, 100, 0, {("tn_w7", 4): 1}),
    case("tn", 300, 200, 100, 0, {("tn_w7", 4): 1}, pad=True),
    case("tn", 2049, 600, 200, 0, {("tn_split", 7): 1}, pad=True),
]
for _M in (0, 1, 15, 17, 2047, 2049):
    TN.append(case("tn", _M, 200, 200, 0, {("tn_split", 7): 1}))
    TN.append(case("tn", _M, 200, 100, 0, {("tn_w7", 4): 1}))
TN = tuple(TN)

ALL = tuple(PANEL) + WRES + SPLIT + TN
assert len({c.id for c in ALL}) == len(ALL), "case ids must be unique"
