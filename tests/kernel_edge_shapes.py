"""The shapes at which tests/test_gpu_gm_kernels.py and
tests/test_gpu_scaler_kernels.py run the kernels of dkm_gm.hip and
dkm_scale.hip, each named for the branch of the plan it is to reach.  Not a
test module: tests/test_kernel_plans_host.py asserts on the CPU, with the
plan restated in dislib_amd/_device.py, that every shape reaches its branch,
and pins that restatement to the library's own workspace sizes."""
import numpy as np

from dislib_amd import _device as dv

ROWS = dv.GM_CHUNK_ROWS

# --- dkm_gm.hip ------------------------------------------------------------
# M-step chunk folding: 16, 17, 18 and 34 chunks; fold_parts takes chunks
# s, s + 16, ... in 16 slices, so every slice is used and the slices take
# one, two and three trips
FOLD_N = [16 * ROWS, 16 * ROWS + 1, 17 * ROWS + 1, 33 * ROWS + 5]
FOLD_CHUNKS = [16, 17, 18, 34]
FOLD_DK = [(3, 3), (17, 2)]
# E-step block counts at (d, K) = (2, 2): 133 blocks, and 257 blocks -- the
# final sum's strided loop takes a second trip
ESTEP_DK = (2, 2)
ESTEP_N = [33 * ROWS + 5, dv.GM_BLOCK * 128 + 1]

# the chunk cap: exactly GM_MAX_CHUNKS chunks of 512 rows; one row more (516
# rows a chunk, the trailing chunks empty); chunks of 520 rows, the last one
# short
CAP_N = [dv.GM_MAX_CHUNKS * ROWS, dv.GM_MAX_CHUNKS * ROWS + 1,
         dv.GM_MAX_CHUNKS * 516 + 3]
CAP_DK = [(1, 1), (2, 2)]

# the covariance workspace cap below the sums' chunking: (d, K, n)
COV_CAP = [(1, 4096, 4100), (17, 1366, 4100)]

# E-step register layouts (d <= 16, 32, 64, 128 in registers, streamed
# beyond) with two K each; every K of {15, 31, 32, 33, 49} at least twice
LAYOUT_DK = [(31, 33), (31, 49), (32, 32), (32, 49), (48, 31), (48, 33),
             (63, 15), (63, 49), (127, 15), (127, 33), (128, 31), (128, 32),
             (130, 15), (130, 33), (131, 31), (131, 32), (144, 15),
             (144, 49), (257, 15), (257, 31)]
LAYOUT_D = [31, 32, 48, 63, 127, 128, 130, 131, 144, 257]
LAYOUT_K = [15, 31, 32, 33, 49]

LOWER_D = [5, 33, 65, 129]
# one shape per layout (d <= 16, <= 32, <= 64, <= 128, streamed)
PER_LAYOUT_DK = [(5, 4), (31, 17), (63, 3), (127, 2), (131, 3)]
NONFINITE_DK = [(5, 4), (33, 17)]

ONEHOT_NK = [(0, 3), (1, 1), (255, 1), (257, 1), (100, 17), (513, 33)]
ONEHOT_GRID_CAP = 65536
# past the grid cap: the stride loop takes a second trip
ONEHOT_BIG = (ONEHOT_GRID_CAP * dv.GM_BLOCK // 7 + 3, 7)


def gm_layout(d):
    """The E-step's register layout of d columns: the columns it keeps in
    registers, 0 for the streamed one."""
    for top in (16, 32, 64, 128):
        if d <= top:
            return top
    return 0


# --- dkm_scale.hip ---------------------------------------------------------
SC_B = 256          # column pieces a block takes per chunk

# column chunks: (dtype, d, pad, pieces of a row, chunks, pieces of the last)
CHUNKS = [
    (np.float64, 257, 1, 257, 2, 1), (np.float32, 257, 1, 257, 2, 1),
    (np.float64, 300, 1, 300, 2, 44), (np.float32, 300, 1, 300, 2, 44),
    (np.float64, 513, 1, 513, 3, 1), (np.float32, 513, 1, 513, 3, 1),
    (np.float64, 514, 0, 257, 2, 1), (np.float32, 1028, 0, 257, 2, 1),
    (np.float64, 1024, 0, 512, 2, 256)]


def scale_pieces(dtype, d, pad):
    """Column pieces of a row on the path (d, d + pad) takes from an
    aligned base: 16 B where both allow, one element otherwise."""
    v = 16 // np.dtype(dtype).itemsize
    return d // v if d % v == 0 and (d + pad) % v == 0 else d


def scale_chunk_sizes(dtype, d, pad):
    """Subset sizes around the row tiles of the first and of the last
    column chunk, an empty Subset, and rows for three blocks."""
    cv = scale_pieces(dtype, d, pad)
    last = cv - (cv - 1) // SC_B * SC_B
    sizes = []
    for r in (dv.SCALE_CHAIN_TILE, SC_B // min(SC_B, cv) * 4,
              SC_B // last * 4):
        sizes += [r - 1, r, r + 1, 2 * r + 1]
    return sizes + [0, 3 * dv.SCALE_GRID_UNIT // d + 5]


# block counts: (dtype, d, n, blocks)
BLOCKS = [(np.float64, 32, 256 * 512 + 1, 257),
          (np.float32, 32, 256 * 512 + 1, 257),
          (np.float64, 32, 600 * 512, 600),
          (np.float32, 32, 600 * 512, 600)]
# the grid cap, the rows of a block not dividing n: just over the cap, and
# one block's rows more than the cap's
CAPPED = [(np.float32, 64, 2048 * 16384 // 64 + 1),
          (np.float32, 64, 2049 * 16384 // 64)]

# wide d: the final sum's grid is min(d, 65535), its blocks take columns
# j, j + 65535, ...
WIDE = [(65537, 5), (65536 + 300, 3)]
FINAL_GRID = 65535
