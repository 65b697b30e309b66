"""CPU tests of the plan restatements in dislib_amd/_device.py (gm_sums_chunks,
gm_cov_chunks, scale_grid and the workspace sizes): every shape of
tests/kernel_edge_shapes.py reaches the branch of dkm_gm.hip / dkm_scale.hip
it is named for, and the restatement gives the library's own workspace
sizes (host-only calls: no GPU)."""
import numpy as np

from dislib_amd import _device as dv
from dislib_amd import _lib
from tests import kernel_edge_shapes as es


def trips(parts, width):
    """Trips of a loop p, p + width, ... over ``parts`` partials, per lane:
    (most, fewest)."""
    return (parts + width - 1) // width, parts // width


def test_gm_fold_shapes_use_every_slice_for_one_two_and_three_trips():
    assert [dv.gm_sums_chunks(n) for n in es.FOLD_N] == es.FOLD_CHUNKS
    assert [trips(c, 16) for c in es.FOLD_CHUNKS] == \
        [(1, 1), (2, 1), (2, 1), (3, 2)]
    for n in es.FOLD_N:
        for d, k in es.FOLD_DK:
            # the covariances fold the same chunks here
            assert dv.gm_cov_chunks(n, d, k) == dv.gm_sums_chunks(n) >= 16
            # no chunk is empty
            per = dv.gm_chunk_rows(n, dv.gm_sums_chunks(n))
            assert per % 4 == 0 and (dv.gm_sums_chunks(n) - 1) * per < n


def test_gm_estep_shapes_reach_the_final_sums_second_trip():
    d, _ = es.ESTEP_DK
    blocks = [dv.gm_estep_blocks(n, d) for n in es.ESTEP_N]
    assert blocks == [133, 257]
    assert trips(blocks[0], dv.GM_BLOCK) == (1, 0)
    assert trips(blocks[1], dv.GM_BLOCK) == (2, 1)


def test_gm_cap_shapes_reach_the_chunk_cap():
    empty = []
    for n in es.CAP_N:
        assert dv.gm_sums_chunks(n) == dv.GM_MAX_CHUNKS
        for d, k in es.CAP_DK:
            assert dv.gm_cov_chunks(n, d, k) == dv.GM_MAX_CHUNKS
        per = dv.gm_chunk_rows(n, dv.GM_MAX_CHUNKS)
        used = (n + per - 1) // per
        empty.append((per, dv.GM_MAX_CHUNKS - used, n - (used - 1) * per))
    # (rows of a chunk, empty trailing chunks, rows of the last used chunk)
    assert empty == [(512, 0, 512), (516, 15, 65), (520, 15, 131)]
    assert dv.gm_sums_chunks(es.CAP_N[0] - 1) == dv.GM_MAX_CHUNKS
    assert dv.gm_sums_chunks(es.CAP_N[0] - 512) == dv.GM_MAX_CHUNKS - 1


def test_gm_cov_cap_shapes_fall_below_the_sums_chunking():
    for d, k, n in es.COV_CAP:
        sums, cov = dv.gm_sums_chunks(n), dv.gm_cov_chunks(n, d, k)
        assert (sums, cov) == (9, 8)
        # chunk_rows rounded up to a multiple of 4, with rows to spare
        per = dv.gm_chunk_rows(n, cov)
        assert per == 516 and per != (n + cov - 1) // cov
        assert (cov - 1) * per < n < cov * per
        # the covariance partials are the workspace
        parts = cov * k * dv.gm_cov_tiles(d) * 2048
        assert dv.gm_workspace_bytes(n, d, k) == parts
    d, k, n = es.COV_CAP[0]
    assert dv.gm_cov_tiles(d) == 1 and \
        dv.gm_workspace_bytes(n, d, k) == dv.GM_COV_WORKSPACE
    d, k, n = es.COV_CAP[1]
    assert dv.gm_cov_tiles(d) == 3
    # the cap itself (7 chunks) is below the floor of 8
    assert dv.GM_COV_WORKSPACE // (k * 3 * 2048) == 7
    # rows that leave the trailing chunks empty at the rounded-up size
    assert dv.gm_chunk_rows(4100, 8) * 8 - 4100 == 28


def test_gm_layout_shapes_cover_every_layout_end_and_every_trip_count():
    assert sorted({d for d, _ in es.LAYOUT_DK}) == es.LAYOUT_D
    assert sorted({k for _, k in es.LAYOUT_DK}) == es.LAYOUT_K
    for d in es.LAYOUT_D:
        assert sum(1 for e, _ in es.LAYOUT_DK if e == d) == 2
    for k in es.LAYOUT_K:
        assert sum(1 for _, e in es.LAYOUT_DK if e == k) >= 2
    assert [es.gm_layout(d) for d in es.LAYOUT_D] == \
        [32, 32, 64, 64, 128, 128, 0, 0, 0, 0]
    # the streamed sizes: d % 4 in {0, 2, 3}, d % 16 == 0, d > 256
    streamed = [d for d in es.LAYOUT_D if es.gm_layout(d) == 0]
    assert {d % 4 for d in streamed} >= {0, 2, 3}
    assert any(d % 16 == 0 for d in streamed) and max(streamed) > 256
    # the second part's lanes: k = c, c + 16, ... takes up to 4 trips
    assert [trips(k, 16)[0] for k in es.LAYOUT_K] == [1, 2, 2, 3, 4]
    assert sorted(es.gm_layout(d) for d, _ in es.PER_LAYOUT_DK) == \
        [0, 16, 32, 64, 128]
    assert sorted(es.gm_layout(d) for d in es.LOWER_D) == [0, 16, 64, 128]
    for d in (63, 64, 65, 128, 129):
        assert dv.gm_estep_block(d) == (64 if es.gm_layout(d) == 128
                                        else 128)


def test_gm_onehot_shapes_pass_the_grid_cap():
    n, k = es.ONEHOT_BIG
    blocks = (n * k + dv.GM_BLOCK - 1) // dv.GM_BLOCK
    assert blocks > es.ONEHOT_GRID_CAP
    assert n * k * 8 < 1 << 30
    for n, k in es.ONEHOT_NK:
        assert (n * k + dv.GM_BLOCK - 1) // dv.GM_BLOCK < es.ONEHOT_GRID_CAP


def test_scale_chunk_shapes_take_their_column_chunks():
    for dtype, d, pad, cv, chunks, last in es.CHUNKS:
        assert es.scale_pieces(dtype, d, pad) == cv
        assert (cv + es.SC_B - 1) // es.SC_B == chunks >= 2
        assert cv - (chunks - 1) * es.SC_B == last
        vector = cv != d
        assert dv.scale_row_tile(d, dtype, vector) == 4
        sizes = es.scale_chunk_sizes(dtype, d, pad)
        # the last chunk's row tile: rp x SC_U rows
        tile = es.SC_B // last * 4
        assert {tile - 1, tile, tile + 1, 2 * tile + 1, 0, 3, 4, 5} <= \
            set(sizes)
        assert dv.scale_grid(sum(sizes), d) >= 3
    assert {c[5] for c in es.CHUNKS} == {1, 44, 256}


def test_scale_block_shapes_reach_their_grids():
    for dtype, d, n, blocks in es.BLOCKS:
        assert dv.scale_grid(n, d) == blocks > es.SC_B
    assert {b[3] for b in es.BLOCKS} == {257, 600}
    for dtype, d, n in es.CAPPED:
        work = (n * d + dv.SCALE_GRID_UNIT - 1) // dv.SCALE_GRID_UNIT
        assert work > dv.SCALE_GRID_CAP == dv.scale_grid(n, d) == 2048
        # 257 rows a block: the last used block is short, the blocks after
        # it are empty
        per = (n + 2047) // 2048
        assert per == 257 and n % per != 0 and (n + per - 1) // per < 2048
        assert n * d * np.dtype(dtype).itemsize < 1 << 28
    assert dv.scale_grid(es.CAPPED[0][2] - 1, 64) == 2048
    assert dv.scale_grid(es.CAPPED[0][2] - 1 - 256, 64) == 2047
    assert dv.scale_grid(0, 64) == 0 and dv.scale_grid(1, 1) == 1


def test_scale_wide_shapes_pass_the_final_sums_grid():
    for d, n in es.WIDE:
        assert d > es.FINAL_GRID and dv.scale_grid(n, d) > 1
        assert trips(d, es.FINAL_GRID) == (2, 1)


def test_restatements_give_the_librarys_workspace_sizes():
    so = _lib.load()
    # each of the three terms of the GaussianMixture workspace largest in
    # turn: the E-step's block partials, the sums', the covariances'
    n = 1 << 27
    assert dv.gm_estep_blocks(n, 1) * 8 == 8 << 20 > \
        dv.gm_cov_chunks(n, 1, 1) * 2048
    assert so.dkm_gm_workspace_bytes(n, 1, 1) == \
        dv.gm_workspace_bytes(n, 1, 1) == 8 << 20
    n, k = dv.GM_MAX_CHUNKS * dv.GM_CHUNK_ROWS, 4096
    sums = dv.GM_MAX_CHUNKS * k * 2 * 8
    assert sums > dv.gm_cov_chunks(n, 1, k) * k * 2048 == 64 << 20
    assert so.dkm_gm_workspace_bytes(n, 1, k) == \
        dv.gm_workspace_bytes(n, 1, k) == sums
    for d, k, n in es.COV_CAP:
        cov = 8 * k * dv.gm_cov_tiles(d) * 2048
        assert so.dkm_gm_workspace_bytes(n, d, k) == \
            dv.gm_workspace_bytes(n, d, k) == cov
    # and every shape the GPU tests run
    shapes = [(n, d, k) for n in es.FOLD_N + es.CAP_N + es.ESTEP_N
              for d, k in es.FOLD_DK + es.CAP_DK]
    shapes += [(n, d, k) for d, k in es.LAYOUT_DK for n in (0, 1, 517)]
    for n, d, k in shapes:
        assert so.dkm_gm_workspace_bytes(n, d, k) == \
            dv.gm_workspace_bytes(n, d, k) > 0, (n, d, k)
    shapes = [(n, d) for _, d, n, _ in es.BLOCKS]
    shapes += [(n, d) for _, d, n in es.CAPPED] + [(n, d) for d, n in es.WIDE]
    shapes += [(sum(es.scale_chunk_sizes(t, d, p)), d)
               for t, d, p, _, _, _ in es.CHUNKS] + [(0, 5), (1, 1)]
    for n, d in shapes:
        assert so.dkm_scale_workspace_bytes(n, d) == \
            dv.scale_workspace_bytes(n, d) > 0, (n, d)
    n, d = es.CAPPED[0][2], 64
    assert dv.scale_workspace_bytes(n, d) == 2048 * 64 * 8
