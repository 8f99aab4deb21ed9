"""The depth build picks its code by size -- one- or two-launch table scans (more than 8 table blocks = 32 768 tiles), atomic or
radix event bucketing (2^20 intervals), a range's events staged in LDS or scattered (28 672 events), the counting join's contig
tables in LDS or in memory (256 contigs) -- and the seam tests' layouts are small on every count.  Here each of those paths runs
in its other form, at the smallest layout that reaches it, against tests/depth_ref.py.  Every test first asserts, from the
reference alone, that its input has the shape it exists for."""
import gzip

import numpy as np
import pytest
import torch

import depth_cases
import depth_ref as R
from gci_amd import pipeline, synth
from gci_amd._lib import GciError
from gci_amd.device import JoinInput

pytestmark = pytest.mark.gpu

TILE = R.TILE


@pytest.fixture(params=["atomic", "radix"])
def events_mode(request, monkeypatch):
    """Both ways a depth build buckets its events by tile (as in test_gpu_seams.py): GCI_EVENTS forces one."""
    monkeypatch.setenv("GCI_EVENTS", request.param)
    return request.param


def _ivl4(rows):
    out = np.zeros((rows.shape[0], 4), dtype=np.int32)
    out[:, :3] = rows
    return out


def _text_bytes_per_base(depth):
    """Bytes of f'{d}\\n' per base."""
    return np.searchsorted(np.array([10, 100, 1000, 10_000, 100_000, 1_000_000], dtype=np.int64), depth, side="right") + 2


def _names(n):
    return ["c%d" % i for i in range(n)]


# ==============================================================================================
# (a) three ranges, mixed staging
# ==============================================================================================

THREE_SETTINGS = [(0, -1, 0), (15, 0, 2)]                    # (flank, lo, hi): issues are lo < depth <= hi


@pytest.fixture(scope="module")
def three(oracle):
    """Per setting: the intervals, the reference, and what the oracle makes of the reference's depths -- computed once for both
    event modes and never written to."""
    lengths = depth_cases.THREE_RANGES_LENGTHS
    names = _names(len(lengths))
    out = {}
    for fl, lo, hi in THREE_SETTINGS:
        rows = depth_cases.three_ranges(fl)
        ref = R.build(lengths, rows, fl)
        depths = {t: R.contig(ref, c) for c, t in enumerate(names)}
        again = rows[::-2]                                    # the second build on the same context: another set, another flank
        out[fl] = dict(rows=rows, ref=ref, track=R.padded_track(ref), text=[oracle.depth_text_contig(depths[t]) for t in names],
                       bed=oracle.collapse_depth_range(depths, lo, hi, fl, 0), again=again,
                       again_track=R.padded_track(R.build(lengths, again, 3)))
    return out


def _assert_three_ranges_shape(rows, ref):
    n_tiles = int(ref.tile_first[-1])
    ev, rng_ev = ref.tile_events, ref.range_events
    assert -(-n_tiles // R.RANGE_TILES) == 3 == rng_ev.shape[0]                           # evp_nb
    assert -(-rows.shape[0] // R.EVP_CHUNK) >= 3                                          # evp_wg
    first = np.concatenate(([0], np.cumsum(rng_ev)))[:-1]                                 # evt_off of a range's first tile
    staged = [r for r in range(3) if 0 < rng_ev[r] <= R.STAGE_CAP]
    assert any(rng_ev[r] > R.STAGE_CAP for r in range(3)) and staged
    for parity in (0, 1):                                                                 # even start: no head; odd start: a head
        of = [r for r in staged if first[r] % 2 == parity]
        assert of, parity
        assert any((rng_ev[r] - parity) % 2 == 1 for r in of), parity                     # an odd tail behind the dwords
    assert (ev <= 30).any() and ((ev > 30) & (ev <= 62)).any() and (ev > 62).any()
    # the layout: a contig boundary inside a range, contigs over both range seams, lengths on and off a tile boundary, contigs
    # without a base in the middle and at the end
    tf, L = ref.tile_first, ref.lengths
    assert any(0 < t % R.RANGE_TILES for t in tf[1:-1])
    for seam in (1024, 2048):
        assert any(tf[c] < seam < tf[c + 1] for c in range(L.shape[0]))
    assert any(x and x % TILE == 0 for x in L) and any(x % TILE for x in L)
    assert L[-1] == 0 and 0 in L[1:-1]
    # intervals: a start in one range and the stop in another; a stop at the contig's end with and without tail padding, one of
    # them with its start in another range than the contig's last tile; 15 000 short ones inside one range
    c, s, e = rows[:, 0], rows[:, 1], rows[:, 2]
    live = (c >= 0) & (c < L.shape[0])
    c, s, e = c[live], s[live], e[live]
    fl = ref.flank
    a, b = R.slice_bound(s + fl, L[c]), R.slice_bound(e - fl + 1, L[c])
    ok = a < b
    ra, rb = (tf[c] + a // TILE) // R.RANGE_TILES, (tf[c] + np.minimum(b, L[c] - 1) // TILE) // R.RANGE_TILES
    assert (ok & (b < L[c]) & (ra != rb)).sum() >= 50
    to_end = ok & (b == L[c])
    assert (to_end & (L[c] % TILE == 0)).any() and (to_end & (L[c] % TILE != 0)).any()
    assert (to_end & (ra != rb) & (L[c] % TILE == 0)).any() and (to_end & (ra != rb) & (L[c] % TILE != 0)).any()
    assert max(int((ok & (b - a <= 800) & (ra == r) & (rb == r)).sum()) for r in range(3)) >= 15_000


@pytest.mark.parametrize("setting", THREE_SETTINGS, ids=lambda s: "flank%d" % s[0])
def test_three_ranges_mixed_staging(engine, oracle, three, events_mode, setting):
    """~2 060 tiles = three ranges of the radix partition, three workgroups of intervals: a [3][3] histogram; range 1 too full
    for the staging area (scattered), ranges 0 and 2 staged with an even and an odd first event index; intervals and the
    event-less coarse -1 of a read that reaches its contig's end across the range seams."""
    fl, lo, hi = setting
    case = three[fl]
    rows, ref = case["rows"], case["ref"]
    _assert_three_ranges_shape(rows, ref)
    lengths = depth_cases.THREE_RANGES_LENGTHS
    names = _names(len(lengths))
    tl = dict(zip(names, lengths))
    engine.set_layout(lengths)
    d = engine.to_device(_ivl4(rows))
    track = engine.new_track()
    out = engine.depth_build_fused(d, None, fl, track, want_text=True, want_sums=True, issue=(lo, hi, fl), want_runs=True)
    members = [bytes(m) for m in engine.depth_deflate(track, from_build=True)]    # from the run lists the build kept
    assert np.array_equal(track.cpu().numpy(), case["track"])                     # the whole buffer, padding included
    assert np.array_equal(out["sums"], ref.sums)
    host_text = out["text"].cpu().numpy().tobytes()
    toff = [int(x) for x in out["text_off"]]
    assert toff == np.concatenate(([0], np.cumsum([len(t) for t in case["text"]]))).tolist()
    for c in range(len(lengths)):
        assert host_text[toff[c]:toff[c + 1]] == case["text"][c], c
        assert (gzip.decompress(members[c]) if members[c] else b"") == case["text"][c], c
    raw = engine.issue_scan(track, lo, hi, fl)
    for c in range(len(lengths)):
        assert np.array_equal(np.asarray(out["runs"][c]), np.asarray(raw[c])), c
    tr = pipeline.DepthTracks(engine, tl, track)
    tr._fresh_runs = ((float(lo), float(hi), fl), out["runs"])
    fused_bed = pipeline.collapse_depth_range(tr, lo, hi, fl, 0)
    tr.invalidate()
    assert fused_bed == pipeline.collapse_depth_range(tr, lo, hi, fl, 0) == case["bed"]
    assert sum(len(v) for v in case["bed"].values()) > 20
    # the per-tile table was left clean: another interval set through the same context
    t2 = engine.new_track()
    engine.depth_build(engine.to_device(_ivl4(case["again"])), None, 3, t2)
    assert np.array_equal(t2.cpu().numpy(), case["again_track"])


# ==============================================================================================
# (b) more than eight table blocks, 30 000 contigs, the production size rule
# ==============================================================================================

MANY_SETTING = (15, -1, 0)


@pytest.fixture(scope="module")
def many(oracle):
    lengths, rows = depth_cases.many_tiles()
    fl = MANY_SETTING[0]
    ref = R.build(lengths, rows, fl)
    csum = np.concatenate(([0], np.cumsum(_text_bytes_per_base(ref.depth))))
    # contig text carries no header: the text of the concatenation is the concatenation of the texts
    return dict(lengths=lengths, rows=rows, ref=ref, track=R.padded_track(ref), text=oracle.depth_text_contig(ref.depth),
                text_off=csum[ref.off])


def _assert_many_tiles_shape(rows, ref, flank):
    tf, L, ev = ref.tile_first, ref.lengths, ref.tile_events
    n_tiles, n = int(tf[-1]), rows.shape[0]
    assert n_tiles > 8 * R.TABLE_BLOCK == 32_768                                          # nb > FEW_BLOCKS
    assert n >= 1 << 20                                                                   # gci_evp_wanted by its own rule
    assert -(-n_tiles // R.RANGE_TILES) * -(-n // R.EVP_CHUNK) > 4096                     # the histogram's scan: several blocks
    starts = np.bincount(tf[:-1][L > 0] // R.TABLE_BLOCK)
    assert starts.max() >= 1000
    # carry-in at the first tile of a table block: the depth of the base in front of it, when that base is of the same contig
    carry = []
    for blk in range(1, -(-n_tiles // R.TABLE_BLOCK)):
        t0 = blk * R.TABLE_BLOCK
        c = int(np.searchsorted(tf, t0, side="right")) - 1
        pos = (t0 - int(tf[c])) * TILE
        carry.append(int(ref.depth[ref.off[c] + pos - 1]) if 0 < pos < L[c] else 0)
    assert sum(1 for x in carry if x > 0) >= 1 and carry[7] > 0                           # ... the one at tile 32 768 among them
    assert (ev[32_768:] > 62).any() and (ev <= 30).any() and ((ev > 30) & (ev <= 62)).any()
    assert (ref.range_events > R.STAGE_CAP).any() and ((ref.range_events > 0) & (ref.range_events <= R.STAGE_CAP)).any()
    assert (L == 0).sum() > 50 and L.shape[0] > 30_000 and (L == 1024 * TILE).any() and (L == 5 * TILE + 1).any()
    assert 0 < L[-1] < 200 and int(ref.sums[-1]) > 0
    # a read's carry crosses many tiles
    assert ((rows[:, 2] - rows[:, 1]) > 4 * TILE).sum() > 1000


@pytest.mark.parametrize("events", ["by_size", "atomic"])
def test_many_table_blocks_and_the_size_rule(engine, oracle, many, monkeypatch, events):
    """33 872 tiles = nine table blocks: the two-launch scans (k_scan2_local / k_scan2_add, device_exclusive_scan over the text
    sizes, gci_launch_reduce_tiles, gci_launch_contig_text_off); 2^20 + 3000 intervals: with GCI_EVENTS unset the radix partition
    by the size rule itself, 34 ranges x 129 workgroups."""
    if events == "by_size":
        monkeypatch.delenv("GCI_EVENTS", raising=False)
    else:
        monkeypatch.setenv("GCI_EVENTS", "atomic")
    fl, lo, hi = MANY_SETTING
    lengths, rows, ref = many["lengths"], many["rows"], many["ref"]
    _assert_many_tiles_shape(rows, ref, fl)
    nc = lengths.shape[0]
    engine.set_layout(lengths)
    d = engine.to_device(_ivl4(rows))
    track = engine.new_track()
    out = engine.depth_build_fused(d, None, fl, track, want_text=True, want_sums=True, issue=(lo, hi, fl))
    assert np.array_equal(track.cpu().numpy(), many["track"])                     # one copy, one comparison, padding included
    assert np.array_equal(out["sums"], ref.sums)
    assert np.array_equal(out["text_off"], many["text_off"])
    assert out["text"].cpu().numpy().tobytes() == many["text"]
    raw = engine.issue_scan(track, lo, hi, fl)
    assert len(raw) == len(out["runs"]) == nc
    assert all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(out["runs"], raw))
    assert sum(len(r) for r in raw) > 1000
    # the seams that share the large-table code, on the same track
    text, toff = engine.depth_text(track)
    assert np.array_equal(np.asarray(toff, dtype=np.int64), many["text_off"])
    assert torch.equal(text[:int(toff[nc])], out["text"])
    tr = pipeline.DepthTracks(engine, dict(zip(_names(nc), lengths.tolist())), track)
    assert np.array_equal(tr.sums(), ref.sums)


# ==============================================================================================
# (c) the counting join beyond 256 contigs
# ==============================================================================================

@pytest.fixture(params=["classic", "partition"])
def join_mode(request, engine):
    engine.set_join_mode(request.param)
    yield request.param
    engine.set_join_mode("auto")


@pytest.fixture(scope="module")
def many_contigs(oracle):
    """300 contigs, most of a few kb, one of 1030 tiles at index 150; two files of reads (the second a perturbed view of the
    first), thinned on the long contig so that the streams stay small.  -> lengths, [(stream, offsets)], what the reference's
    join keeps as sorted (contig, start, end)."""
    rng = np.random.default_rng(300)
    lengths = rng.integers(2000, 9000, 300)
    lengths[150] = 1030 * TILE + 123
    contigs = tuple(("k%03d" % i, int(l)) for i, l in enumerate(lengths))
    targets = [n for n, _ in contigs]
    a = synth.simulate_reads(contigs, 30, "hifi", seed=301)
    on_long = np.flatnonzero(a.ref_id == 150)
    a = a.take(np.sort(np.concatenate([np.flatnonzero(a.ref_id != 150), on_long[::6]])))
    sets = [a, synth.perturb(a, 302)]
    streams, dicts, hq = [], [], set()
    for rs in sets:
        stream, offs = synth.to_bam_stream(rs)
        d, h = oracle.bam_file_dict(stream, offs, targets, targets, 30, 50, 0.1, 0.9)
        streams.append((stream, offs))
        dicts.append(d)
        hq |= h
    tindex = {t: i for i, t in enumerate(targets)}
    want = sorted((tindex[v[0]], v[1], v[2]) for v in oracle.name_join(dicts, hq, 0.9).values())
    return [int(x) for x in lengths], streams, want


def test_counting_join_beyond_256_contigs(engine, oracle, many_contigs, join_mode, events_mode):
    """test_counting_join_equals_join_then_count (test_gpu_seams.py) on 300 contigs: gci_name_join_count reads the contig tables
    from memory, not from its 256-entry copies in LDS.  Counted build == join-then-build == the reference on the reference's
    intervals."""
    lengths, streams, want = many_contigs
    nc, flank = len(lengths), 15
    used = set(c for c, _, _ in want)
    assert nc > 256 and len(used) >= 200 and sum(1 for c in used if c >= 256) >= 20 and 150 in used
    assert -(-lengths[150] // TILE) > 1024
    ref = R.build(lengths, np.asarray(want, dtype=np.int64), flank)
    want_track = R.padded_track(ref)
    engine.set_layout(lengths)
    files = []
    for stream, offs in streams:
        d_bam, d_off = engine.to_device(stream), engine.to_device(offs)
        recs = engine.bam_filter(d_bam, d_off, engine.to_device(np.arange(nc, dtype=np.int32)), 30, 50, 0.1, 0.9)
        files.append(JoinInput(recs, d_bam, d_off, 36))
    results = []
    for fused in (False, True):
        ivl, cnt = engine.name_join(files, 0.9, count_flank=flank if fused else None)
        n = int(cnt.item())
        assert sorted(map(tuple, ivl[:n, :3].cpu().numpy().tolist())) == want
        track = engine.new_track()
        out = engine.depth_build_fused(ivl, cnt, flank, track, want_text=True, want_sums=True, issue=(-1, 0, flank), counted=fused)
        results.append((track.cpu().numpy(), out["text"].cpu().numpy().tobytes(), out["sums"].tolist(),
                        [np.asarray(r).tolist() for r in out["runs"]]))
    assert np.array_equal(results[0][0], want_track) and results[0][2] == ref.sums.tolist()
    assert np.array_equal(results[1][0], want_track) and results[1][1:] == results[0][1:]
    assert results[0][1] == oracle.depth_text_contig(ref.depth)
    # a counted build with another flank is refused, and the table is clean again for a plain build
    ivl, cnt = engine.name_join(files, 0.9, count_flank=flank)
    with pytest.raises(GciError):
        engine.depth_build_fused(ivl, cnt, 3, engine.new_track(), want_text=False, counted=True)
    t2 = engine.new_track()
    engine.depth_build(ivl, cnt, flank, t2)
    assert np.array_equal(t2.cpu().numpy(), want_track)
