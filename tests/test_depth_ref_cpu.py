"""tests/depth_ref.py (the vectorised statement the depth build is held to in test_gpu_build_shapes.py) against the oracle's two
restatements of GCI.py:302-306 -- depth_build_py, the literal numpy slice, and depth_build, the compiled loop -- and its event
counts against a per-interval loop written here, on the interval sets of the seam tests: negative-stop wraps, empty slices,
reads hanging over the end, contigs of one base."""
import numpy as np
import pytest

import depth_cases
import depth_ref as R

FLANKS = (0, 3, 15, 5000)
CASES = {"slice_semantics": depth_cases.slice_semantics, "sparse_dense_1": lambda: depth_cases.sparse_and_dense(1),
         "sparse_dense_2": lambda: depth_cases.sparse_and_dense(2), "sparse_dense_3": lambda: depth_cases.sparse_and_dense(3)}


@pytest.fixture(scope="module", params=list(CASES))
def case(request):
    lengths, ivls = CASES[request.param]()
    return lengths, ivls


def _py_bound(v, L):
    return slice(v, None).indices(L)[0]              # the interpreter's own rule for a slice bound


def _events_loop(lengths, ivls, flank):
    """k_evt_count's events, one interval at a time: one in the tile of the start, one in the tile of the stop unless the stop is
    the end of a contig that ends on a tile boundary."""
    L = list(lengths)
    tf = [0]
    for x in L:
        tf.append(tf[-1] + -(-x // R.TILE))
    ev = [0] * tf[-1]
    for c, s, e in ivls:
        a, b = _py_bound(s + flank, L[c]), _py_bound(e - flank + 1, L[c])
        if a >= b:
            continue
        ev[tf[c] + a // R.TILE] += 1
        if b < -(-L[c] // R.TILE) * R.TILE:
            ev[tf[c] + b // R.TILE] += 1
    return tf, ev


@pytest.mark.parametrize("flank", FLANKS)
def test_depths_equal_the_oracles(oracle, case, flank):
    lengths, ivls = case
    targets = list(lengths)
    ref = R.build([lengths[t] for t in targets], ivls, flank)
    literal = oracle.depth_build_py([(targets[c], s, e) for c, s, e in ivls], lengths, flank)
    compiled = oracle.depth_build({i: (targets[c], s, e) for i, (c, s, e) in enumerate(ivls)}, lengths, flank)
    assert ref.depth.dtype == ref.off.dtype == ref.sums.dtype == ref.tile_events.dtype == ref.range_events.dtype == np.int64
    assert ref.off.tolist() == np.concatenate(([0], np.cumsum([lengths[t] for t in targets]))).tolist()
    for c, t in enumerate(targets):
        assert np.array_equal(R.contig(ref, c), literal[t]), (t, flank)
        assert np.array_equal(R.contig(ref, c), compiled[t]), (t, flank)
        assert int(ref.sums[c]) == int(literal[t].sum())
    if flank < 5000:
        assert int(ref.sums.sum()) > 0
    # the padded layout: every contig from its first tile on, zeros between
    track = R.padded_track(ref, np.int64)
    assert track.shape[0] == int(ref.tile_first[-1]) * R.TILE and int(track.sum()) == int(ref.sums.sum())
    for c, t in enumerate(targets):
        o = int(ref.tile_first[c]) * R.TILE
        assert np.array_equal(track[o:o + lengths[t]], literal[t])


@pytest.mark.parametrize("flank", FLANKS)
def test_event_counts_equal_a_loop(case, flank):
    lengths, ivls = case
    ref = R.build(list(lengths.values()), ivls, flank)
    tf, ev = _events_loop(lengths.values(), ivls, flank)
    assert ref.tile_first.tolist() == tf
    assert ref.tile_events.tolist() == ev
    assert ref.range_events.tolist() == [sum(ev[i:i + R.RANGE_TILES]) for i in range(0, len(ev), R.RANGE_TILES)]


def test_slice_bound_is_pythons():
    for L in (0, 1, 5, 4096):
        for v in range(-2 * L - 3, 2 * L + 4):
            assert int(R.slice_bound(v, L)) == _py_bound(v, L), (v, L)


def test_rows_outside_the_layout_and_empty_sets():
    ref = R.build([10, 0, 5000], [(0, 2, 5), (3, 0, 9), (-1, 0, 9), (1, 0, 4), (2, 4090, 6000)], 0)
    assert R.contig(ref, 0).tolist() == [0, 0, 1, 1, 1, 1, 0, 0, 0, 0] and R.contig(ref, 1).shape[0] == 0
    assert ref.sums.tolist() == [4, 0, 910] and ref.tile_first.tolist() == [0, 1, 1, 3]
    assert ref.tile_events.tolist() == [2, 1, 1] and ref.range_events.tolist() == [4]     # 4090 and the stop at 5000, in padding
    none = R.build([7, 4096], [], 15)
    assert none.depth.tolist() == [0] * 4103 and none.tile_events.tolist() == [0, 0]


def test_the_large_cases_are_what_they_claim():
    """The shapes of test_gpu_build_shapes.py's two layouts, as far as they can be seen without the device (the tests there assert
    them again, next to the event counts they are about)."""
    for flank in (0, 15):
        rows = depth_cases.three_ranges(flank)
        ref = R.build(depth_cases.THREE_RANGES_LENGTHS, rows, flank)
        assert int(ref.tile_first[-1]) == 2061 and ref.range_events.shape[0] == 3
        assert -(-rows.shape[0] // R.EVP_CHUNK) >= 3
        assert [int(x) % 2 for x in ref.range_events] == [1, 0, 0]
