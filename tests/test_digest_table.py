"""The digest scan's candidate-mask table: a scan of the plane tests every byte pair by one lookup
in a table of 65 536 bytes, bit j of a byte set when the pair is a key of candidate j, (da, db) or
(da, DIGEST_DEAD), for up to pkg.DIGEST_CAND candidates at once.  The cases are those in which
candidates meet in one byte of the table, or in which the workgroup that fills the table is not
full.  As in test_digest_lists.py every test drives mergeUntil in batches of 8 against the oracle
and requires, after every batch, the oracle's merges and samples and a maintained table equal to a
recount in all 81 920 bins; the W of the placed pairs is checked against the oracle before anything
is asserted about the engine.  Sizes: 1.2 M tokens (two chunks per region: chunk boundaries with an
even index are region boundaries too), and one corpus of 999 chunks, a region each."""
import functools

import numpy as np
import pytest

from bpe_amd import pkg
from test_digest_lists import Cells
from test_digest_stream import CHUNK, HOT_BASE, drive, filler, light_pairs_corpus, n_chunks_of

gpu = pytest.mark.gpu
K = pkg.DIGEST_CAND


def ordered_corpus(first, rest=6, base=HOT_BASE, seed=51):
    """1.2 M tokens over the filler ids 32 .. 199 with the pairs `first` ((a, b, W), heaviest
    first) and `rest` lighter pairs (4, 5), (6, 7), .. after them, every third site of each across
    a chunk boundary; `base` ids."""
    rng = np.random.default_rng(seed)
    buf = filler(rng, 1_200_000, lo=32)
    pl = Cells(rng, buf)
    order = list(first)
    w = min(p[2] for p in first)
    for i in range(rest):
        order.append((4 + 2 * i, 5 + 2 * i, w - 10 * (i + 1)))
    for a, b, cnt in order:
        pl.put([a, b], cnt)
    return [buf, filler(rng, 555, lo=32)], [1] * base, order


def one_batch(monkeypatch, first, base=HOT_BASE):
    """The corpus of `first` driven for one batch: its eight pairs merge in their order, all on
    the plane, and no merge disturbs the table's order, so a scan serves K of them."""
    monkeypatch.delenv('BPE_DIGEST_CAND', raising=False)
    monkeypatch.delenv('BPE_DIGEST', raising=False)
    samples, len16, order = ordered_corpus(first, 8 - len(first), base)
    stats, merges, per_batch = drive(samples, len16, 0, 1, {p[:2] for p in order})
    print(per_batch)
    assert merges == order, merges
    assert stats['digest_passes'] == 8 and stats['digest_builds'] == 1, stats
    assert 1 <= stats['digest_scans'] <= -(-8 // K) + 1, stats
    return stats


# ---- (a) two candidates in one byte -----------------------------------------------------------------
@gpu
def test_candidates_whose_digests_alias_entry_for_entry(monkeypatch):
    """(0, 1) and (254, 255): ids t and t + 254 have one digest, so both keys of the one pair are
    the keys of the other, and the scan for (0, 1) caches (254, 255) with both bits in the same two
    bytes.  Each merge rewrites its own sites alone (the oracle's merges and samples, the recount);
    the other pair's chunks are false hits, which cost loads and nothing else."""
    d = pkg.digest(np.array([0, 1, 254, 255], np.int32))
    assert d[0] == d[2] and d[1] == d[3] and pkg.HOT_BINS == 256 * 256   # (ids below 256 are hot)
    stats = one_batch(monkeypatch, [(0, 1, 280), (254, 255, 270)], base=256)
    assert stats['digest_hits'] >= stats['delta_chunks'], stats
    # (every chunk of either pair is a hit of both merges)
    assert stats['digest_hits'] > stats['delta_chunks'], stats


@gpu
def test_a_candidate_whose_two_digests_are_equal(monkeypatch):
    """(0, 254) and (254, 0): da == db with a != b, the key (da, db) a byte pair of two equal
    bytes; the two candidates share both keys."""
    d = pkg.digest(np.array([0, 254], np.int32))
    assert d[0] == d[1]
    stats = one_batch(monkeypatch, [(0, 254, 280), (254, 0, 270)], base=256)
    assert stats['digest_hits'] >= stats['delta_chunks'], stats


# ---- (b) one second key for two candidates ---------------------------------------------------------
SECTIONS = (('empty', 1, 70), ('empty', 3, 60), ('tail', 1, 60), ('tail', 3, 60))
LIGHT = ((4, 5), (6, 7), (8, 9), (10, 11), (16, 17), (18, 19), (20, 21), (22, 23), (24, 25),
         (26, 27), (28, 29), (30, 31), (0, 2))


def shared_tail_corpus():
    """250 sections: a 14, a run of 256 slots 12 13 12 13 .., then b = 1 (130 sections) or 3 (120).
    Eight heavy merges (full passes) turn each run into one token z; ten more runs without the 14
    keep (z', z') above (14, z') at the last of them.  (14, z) -> u, W 250, follows, and leaves
    u as its chunk's last live token in every section:
      'empty': the 14 in slot 255, the run the whole next chunk: that chunk is empty, u is
               followed by its dead slot 0, and b is slot 0 of the chunk after it;
      'tail':  the 14 in slot 127, the run over the chunk boundary: u is followed by its own
               chunk's dead tail, and b is the first live token of the next chunk.
    Sections lie at chunk boundaries of both parities (inside a region and across two).  Seven
    light pairs (W 240 .. 180) fill the second batch on the stale plane; the third, on a rebuilt
    plane, begins with (u, 1), W 130, and (u, 3), W 120: two candidates of one scan whose second
    key (du, DIGEST_DEAD) is one byte of the table, reached through it in every section.  Six
    lighter pairs (W 112 .. 92) follow."""
    rng = np.random.default_rng(52)
    buf = filler(rng, 1_200_000, lo=32)
    k = 100
    for kind, b, count in SECTIONS + (('plain', 0, 10),):
        for s in range(count):
            c = k + (s & 1)            # the chunk that holds the 14
            k += 8
            start = CHUNK * (c + 1) - (0 if kind != 'tail' else 128)
            buf[start:start + CHUNK] = [12, 13] * (CHUNK // 2)
            if kind != 'plain':
                buf[start - 1] = 14
                buf[start + CHUNK] = b
    assert k <= 2200
    pl = Cells(rng, buf)
    pl.cells = iter([c for c in pl.cells if c > 2210 * 4])
    pl.edges = iter([c for c in pl.edges if c > 2210])
    for i, (x, y) in enumerate(LIGHT):
        pl.put([x, y], 240 - 10 * i if i < 7 else 112 - 4 * (i - 7))
    return [buf, filler(rng, 555, lo=32)], [1] * HOT_BASE


@gpu
def test_two_candidates_with_one_second_key(monkeypatch):
    monkeypatch.delenv('BPE_DIGEST_CAND', raising=False)
    monkeypatch.delenv('BPE_DIGEST', raising=False)
    samples, len16 = shared_tail_corpus()
    u = HOT_BASE + 8
    wanted = {(14, HOT_BASE + 7), (u, 1), (u, 3)} | set(LIGHT)
    stats, merges, per_batch = drive(samples, len16, 0, 3, wanted)
    print(per_batch)
    assert merges[0] == (12, 13, 260 * 128) and merges[7][2] == 260, merges[:8]
    assert merges[8] == (14, HOT_BASE + 7, 250), merges[8]
    assert [m[:2] for m in merges[9:16]] == list(LIGHT[:7]), merges[9:16]
    assert merges[16:18] == [(u, 1, 130), (u, 3, 120)], merges[16:18]
    assert [m[:2] for m in merges[18:]] == list(LIGHT[7:]), merges[18:]
    b1, b2 = per_batch[1], per_batch[2]
    # the third batch runs on a rebuilt plane, and its first merge has no list to take
    assert b2['digest_builds'] == b1['digest_builds'] + 1, per_batch
    assert b2['digest_passes'] - b1['digest_passes'] == 8, per_batch
    assert b2['digest_scans'] - b1['digest_scans'] >= 1, per_batch
    if K > 1:
        assert b2['digest_scans'] - b1['digest_scans'] < 8, per_batch


# ---- (c) eight candidates ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def many_run(cand):
    """24 strictly ordered light pairs on disjoint tokens in three batches, under
    BPE_DIGEST_CAND=cand (None: unset); the caller sets the environment."""
    samples, len16 = light_pairs_corpus(24)
    return drive(samples, len16, 0, 3, {(2 * i, 2 * i + 1) for i in range(24)})


@gpu
def test_one_scan_answers_for_every_slot(monkeypatch):
    monkeypatch.delenv('BPE_DIGEST', raising=False)
    monkeypatch.delenv('BPE_DIGEST_CAND', raising=False)
    stats, merges, per_batch = many_run(None)
    monkeypatch.setenv('BPE_DIGEST_CAND', '1')
    one, merges1, per_batch1 = many_run(1)
    print(per_batch, per_batch1)
    # (the pairs from (32, 33) on are made of filler ids and weigh the background's count more:
    # the 24 are the merges, in the order of their weights, two of which tie, not of their ids)
    assert sorted(m[:2] for m in merges) == [(2 * i, 2 * i + 1) for i in range(24)], merges
    assert all(x[2] >= y[2] for x, y in zip(merges, merges[1:])), merges
    assert stats['digest_passes'] == 24 and stats['digest_builds'] == 1, stats
    assert 1 <= stats['digest_scans'] <= -(-24 // K) + 1, stats
    assert stats['digest_hits'] >= stats['delta_chunks'], stats
    # every iteration scans under the cap of one candidate: the same merges, the same rewrites
    assert one['digest_scans'] == one['digest_passes'] == 24, one
    assert merges1 == merges
    assert one['delta_chunks'] == stats['delta_chunks'], (one, stats)


# ---- (d) a workgroup with fewer regions than waves --------------------------------------------------
@gpu
def test_waves_without_a_region_fill_the_table_and_leave(monkeypatch):
    """999 chunks, a region each: the last workgroup has 7 regions for its 16 waves, and the other
    9 must pass both barriers of the table's fill before they return.  The background of 168 ids
    counts about 9 per pair here; the eight pairs weigh 60 - 4 i (16 W below the chunks)."""
    monkeypatch.delenv('BPE_DIGEST_CAND', raising=False)
    monkeypatch.delenv('BPE_DIGEST', raising=False)
    rng = np.random.default_rng(53)
    buf = filler(rng, 255_000, lo=32)
    pl = Cells(rng, buf)
    order = [(2 * i, 2 * i + 1, 60 - 4 * i) for i in range(8)]
    for a, b, cnt in order:
        pl.put([a, b], cnt)
    samples = [buf, filler(rng, 555, lo=32)]
    nch = n_chunks_of(samples)
    assert nch == 999 and nch % 16 == 7 and 16 * 60 < nch
    stats, merges, per_batch = drive(samples, [1] * HOT_BASE, 0, 1, {p[:2] for p in order})
    print(per_batch)
    assert merges == order, merges
    assert stats['digest_passes'] == 8 and stats['digest_scans'] >= 1, stats
    assert stats['digest_scans'] <= -(-8 // K) + 1, stats
