"""Segmentations that pin every route of temp_segment_sum_rows (temp_amd/csrc/rows_kernels.hip: segment_sum_rows), shared by the
host-side workspace test and the GPU route tests.  A case is a list of segment lengths; the route follows from
(n_seg, n_rows = sum of the lengths, d) alone:

    split   n_rows >= 512 n_seg, S = min(64, 2048 // n_seg) >= 2     two launches, workspace n_seg S d 4 bytes
    pieces  2 n_seg < n_rows <= 32 n_seg                             two launches, workspace ceil(n_rows / 32) 2 d 4 bytes
    blk16   n_rows >= 96 n_seg                                       one launch, no workspace
    blk4    32 n_seg < n_rows < 96 n_seg                             one launch, no workspace
    short   0 < n_rows <= 2 n_seg                                    one launch, no workspace
and d > 256 (more float4 columns than a wave has lanes) takes none of the first four: one launch, no workspace."""
import functools

import numpy as np

WIDE_D = (260, 320, 512)


def _to_total(lens, total):
    """Spread total - sum(lens) evenly over the long segments (the short and empty ones stay as they were set)."""
    big = np.flatnonzero(lens >= 64)
    diff = int(total - lens.sum())
    lens[big] += diff // len(big)
    lens[big[:diff % len(big)]] += 1
    assert lens.sum() == total
    return lens


def _short():
    rng = np.random.default_rng(11)
    lens = rng.choice([0, 1, 2], size=1003, p=[0.2, 0.2, 0.6])
    lens[0], lens[1], lens[-1] = 0, 2, 1
    lens[500] = 40
    return lens


def _pieces():
    """300 segments, ~3000 rows: empty segments first, last and in runs; a segment that fills piece 0 exactly (starts and ends at a
    multiple of 32); one that ends at 64; a 600-row hub from row 64 (19 pieces: the 16-unrolled loop and the tail loop of the
    second kernel); a 70-row segment that starts inside a piece; a partial last piece."""
    rng = np.random.default_rng(12)
    head = [0, 0, 32, 5, 27, 0, 0, 0, 600, 5, 70, 0, 0]
    rest = rng.integers(0, 18, size=300 - len(head) - 2)
    lens = np.array(head + list(rest) + [3, 0], dtype=np.int64)
    if lens.sum() % 32 == 0:
        lens[-2] += 1
    return lens


def _blk4_skew():
    lens = np.zeros(50, dtype=np.int64)
    lens[7] = 1500
    live = [s for s in range(50) if s not in (0, 7, 20, 21, 22, 49)]
    rng = np.random.default_rng(13)
    cut = np.sort(rng.choice(np.arange(1, 1500), size=len(live) - 1, replace=False))
    lens[live] = np.diff(np.concatenate([[0], cut, [1500]]))
    return lens


def _blk4_stride():
    rng = np.random.default_rng(14)
    return 34 + rng.integers(-10, 11, size=4100)


def _blk16():
    rng = np.random.default_rng(15)
    cut = np.sort(rng.choice(np.arange(1, 6000), size=29, replace=False))
    return np.diff(np.concatenate([[0], cut, [6000]]))


def _blk16_many():
    rng = np.random.default_rng(16)
    return _to_total(520 + rng.integers(-200, 201, size=1100), 520 * 1100)


def _split3():
    return np.array([5000, 3, 0], dtype=np.int64)


def _split33():
    rng = np.random.default_rng(17)
    lens = 600 + rng.integers(-500, 501, size=33)
    lens[4] = 0
    return _to_total(lens, 600 * 33)


def _split1024():
    rng = np.random.default_rng(18)
    lens = 512 + rng.integers(-400, 401, size=1024)
    lens[:3] = (0, 1, 2)
    return _to_total(lens, 512 * 1024)


# name -> (segment lengths, route at d <= 256, S of the split route, widths)
_CASES = {
    "short": (_short, "short", 0, (8, 32, 64, 128, 200, 256)),
    "pieces": (_pieces, "pieces", 0, (8, 200, 256)),
    "blk4_skew": (_blk4_skew, "blk4", 0, (32, 200)),
    "blk4_stride": (_blk4_stride, "blk4", 0, (8,)),
    "blk16": (_blk16, "blk16", 0, (256,)),
    "blk16_many": (_blk16_many, "blk16", 0, (8,)),
    "split3": (_split3, "split", 64, (8, 256)),
    "split33": (_split33, "split", 62, (200,)),
    "split1024": (_split1024, "split", 2, (8,)),
}
WIDE_CASES = ("short", "pieces", "blk16", "split3")
NULL_WS_CASES = [("pieces", d) for d in (8, 64, 128, 200)] + [("split3", 8)]
NARROW = [(name, d) for name, c in _CASES.items() for d in c[3]]
WIDE = [(name, d) for name in WIDE_CASES for d in WIDE_D]


@functools.lru_cache(maxsize=None)
def lengths(name):
    lens = np.asarray(_CASES[name][0](), dtype=np.int64)
    assert (lens >= 0).all()
    return lens


def route(name, d):
    return "wide" if d > 256 else _CASES[name][1]


def check_shape(name):
    """The case is what its name says: the thresholds of the dispatch, restated, and the features each route's kernels depend on."""
    lens = lengths(name)
    n_seg, n_rows, kind = len(lens), int(lens.sum()), _CASES[name][1]
    ptr = np.concatenate([[0], np.cumsum(lens)])
    if kind == "short":
        assert 0 < n_rows <= 2 * n_seg and n_seg % 16 != 0 and lens.max() == 40 and set(np.unique(lens)) == {0, 1, 2, 40}
    elif kind == "pieces":
        assert 2 * n_seg < n_rows <= 32 * n_seg and n_rows % 32 != 0
        assert lens[0] == 0 and lens[-1] == 0 and ((lens[:-1] == 0) & (lens[1:] == 0)).any()
        live = lens > 0
        assert ((ptr[:-1] % 32 == 0) & live).any() and ((ptr[1:] % 32 == 0) & live).any()
        hub = int(np.argmax(lens))
        assert lens[hub] == 600 and (ptr[hub + 1] - 1) // 32 - ptr[hub] // 32 >= 17
        assert ((ptr[:-1] % 32 != 0) & (lens > 64)).any()
    elif kind == "blk4":
        assert 32 * n_seg < n_rows < 96 * n_seg
        assert n_seg > 4096 or (lens.max() == 1500 and (lens == 0).any())
    elif kind == "blk16":
        assert 96 * n_seg <= n_rows and (n_rows < 512 * n_seg or n_seg > 1024)
    else:
        S = _CASES[name][2]
        assert kind == "split" and n_rows >= 512 * n_seg and S == min(64, 2048 // n_seg) >= 2
        assert (lens < S).any() and (lens == 0).any()
    return n_seg, n_rows


def workspace_bytes(name, d):
    """What temp_segment_sum_rows_workspace must answer for the case at width d."""
    lens = lengths(name)
    n_seg, n_rows, r = len(lens), int(lens.sum()), route(name, d)
    if r == "split":
        return n_seg * _CASES[name][2] * d * 4
    if r == "pieces":
        return -(-n_rows // 32) * 2 * d * 4
    return 0


def launches(name, d):
    return 2 if route(name, d) in ("split", "pieces") else 1


def gather_ids(name, seed=0):
    """A shuffled gather index list with these segment lengths and ~2 % entries of -1 (rows that belong to no segment)."""
    lens = lengths(name)
    rng = np.random.default_rng(seed + len(lens))
    ids = np.repeat(np.arange(len(lens), dtype=np.int32), lens)
    ids = np.concatenate([ids, np.full(max(1, len(ids) // 50), -1, dtype=np.int32)])
    rng.shuffle(ids)
    return ids
