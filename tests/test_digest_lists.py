"""The hit lists of the digest stream: one stream of the plane answers "can this chunk hold a site?"
for the decided pair and for the predicted next ones (pkg.DIGEST_CAND candidates, capped by
BPE_DIGEST_CAND), and the later merges are applied from the cached lists without another stream.
As in test_digest_stream.py every test drives mergeUntil in batches of 8 against the oracle and
requires, after every batch, the oracle's merges and samples and a maintained table equal to a
recount in all 81 920 bins; the W of the placed pairs is checked against the oracle before anything
is asserted about the engine.  Sizes: 1.2 M tokens (two chunks per region: chunk boundaries with an
even index are region boundaries too), and one case of 36 M tokens whose rows pass one word."""
import functools

import numpy as np
import pytest

from bpe_amd import make_engine, pkg
from oracle import OracleState
from test_digest_stream import (CHUNK, HOT_BASE, Placer, check_table, drive, filler,
                                light_pairs_corpus)

gpu = pytest.mark.gpu
K = pkg.DIGEST_CAND


class Cells:
    """Structures of up to eight tokens, none touching another: `inside` a 64-token cell of its
    own, `across` with its first `left` tokens at the end of a chunk of its own."""

    def __init__(self, rng, buf):
        self.rng, self.buf = rng, buf
        self.cells = iter(rng.permutation(np.arange(8, len(buf) // 64 - 8)))
        self.edges = iter(rng.permutation(np.arange(4, len(buf) // CHUNK - 4)))

    def inside(self, toks):
        pos = int(next(self.cells)) * 64 + int(self.rng.integers(2, 54))
        self.buf[pos:pos + len(toks)] = toks

    def across(self, toks, left):
        pos = int(next(self.edges)) * CHUNK - left
        self.buf[pos:pos + len(toks)] = toks

    def put(self, toks, count, every=3):
        """count copies, every `every`-th across a chunk boundary (cut at each inner position in
        turn)."""
        for i in range(count):
            if every and i % every == 0:
                self.across(toks, 1 + (i // every) % (len(toks) - 1))
            else:
                self.inside(toks)


# ---- (a) reuse -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reuse_run(cand):
    """16 strictly ordered light pairs in two batches, under BPE_DIGEST_CAND=cand (None: unset);
    the caller sets the environment."""
    samples, len16 = light_pairs_corpus(16)
    return drive(samples, len16, 0, 2, {(2 * i, 2 * i + 1) for i in range(16)})


@gpu
def test_later_merges_are_applied_from_the_lists_of_one_scan(monkeypatch):
    monkeypatch.delenv('BPE_DIGEST_CAND', raising=False)
    stats, merges, per_batch = reuse_run(None)
    monkeypatch.setenv('BPE_DIGEST_CAND', '1')
    one, merges1, per_batch1 = reuse_run(1)
    print(per_batch, per_batch1)
    assert [m[:2] for m in merges] == [(2 * i, 2 * i + 1) for i in range(16)], merges
    assert stats['digest_passes'] == 16 and stats['digest_builds'] == 1, stats
    if K > 1:
        assert 0 < stats['digest_scans'] < stats['digest_passes'], stats
        # the pairs' order is the table's order and no merge disturbs it: a scan serves K merges,
        # and a list outlives the batch it was read in
        assert stats['digest_scans'] <= -(-16 // K) + 1, stats
        # a listed chunk is a hit; a scan's hits are the decided pair's alone
        assert stats['digest_hits'] >= stats['delta_chunks'], stats
    # every iteration scans under the cap of one candidate: the same merges, the same rewrites
    assert one['digest_scans'] == one['digest_passes'] == 16, one
    assert merges1 == merges
    assert one['delta_chunks'] == stats['delta_chunks'], (one, stats)


# ---- (b) candidates disturbed by the merge before them ---------------------------------------------
def disturbed_corpus(lone_pa, lone_ba):
    """a, b, p, q = 0, 1, 2, 3.  Triples p a b and a b q (50 each), chains a b a b (35) and 100 lone
    a b: (a, b) W 270, the first merge (16 W stays below the 4690 chunks).  While the plane is
    scanned for it, (p, a) counts 50 + lone_pa, (b, q) 230 and (b, a) 35 + lone_ba; the merge takes
    50, 50 and 35 of them away, and a pair cached by that scan is merged later from a list whose
    triple or chain chunks hold no site of it any more.  (p, a) and (b, a) lie in the same block of
    the table (one block per second id), and the prediction takes one key per block: the heavier
    of the two is cached beside (b, q), the other is scanned for after (a, b).  Four lighter pairs
    follow."""
    rng = np.random.default_rng(41)
    buf = filler(rng, 1_200_000)
    pl = Cells(rng, buf)
    pl.put([2, 0, 1], 50)
    pl.put([0, 1, 3], 50)
    pl.put([0, 1, 0, 1], 35)
    pl.put([0, 1], 100)
    pl.put([2, 0], lone_pa)
    pl.put([1, 3], 180)
    pl.put([1, 0], lone_ba)
    for i, w in enumerate((160, 150, 140, 130)):
        pl.put([4 + 2 * i, 5 + 2 * i], w)
    return [buf, filler(rng, 555)], [1] * HOT_BASE


# lone (p, a), lone (b, a), the merges, and the scans with four candidates:
#  pa_cached: (0, 1) scans for itself, (2, 0), (1, 3) and (4, 5); two merges from those rows;
#             (1, 0) scans for itself, (4, 5), (6, 7), (8, 9); three from those; (10, 11) scans
#  ba_cached: (0, 1) scans for itself, (1, 0), (1, 3) and (4, 5): the chains a b a b are c c when
#             (1, 0) is applied from its row; (6, 7) scans for itself, (2, 0), (8, 9), (10, 11)
DISTURBED = {
    'pa_cached': (190, 170, [(0, 1, 270), (2, 0, 190), (1, 3, 180), (1, 0, 170), (4, 5, 160),
                             (6, 7, 150), (8, 9, 140), (10, 11, 130)], 3),
    'ba_cached': (145, 200, [(0, 1, 270), (1, 0, 200), (1, 3, 180), (4, 5, 160), (6, 7, 150),
                             (2, 0, 145), (8, 9, 140), (10, 11, 130)], 2),
}


@gpu
@pytest.mark.parametrize('case', sorted(DISTURBED))
def test_lists_read_before_a_merge_that_removes_their_sites(monkeypatch, case):
    monkeypatch.delenv('BPE_DIGEST_CAND', raising=False)
    lone_pa, lone_ba, order, scans4 = DISTURBED[case]
    samples, len16 = disturbed_corpus(lone_pa, lone_ba)
    stats, merges, per_batch = drive(samples, len16, 0, 1, {m[:2] for m in order})
    print(per_batch)
    assert merges == order, merges
    assert stats['digest_passes'] == 8, stats
    if K > 1:
        assert stats['digest_scans'] < 8, stats
    if K == 4:
        assert stats['digest_scans'] == scans4, stats


# ---- (c) a prediction miss -------------------------------------------------------------------------
def miss_corpus():
    """260 triples 0 1 3 and 20 lone 0 1: (0, 1) W 280 makes 260 sites of (c, 3), above every pair
    cached beside it ((4, 5) 250, (6, 7) 240, (8, 9) 230; then 220, 210, 200).  (20, 21), W 290,
    goes first."""
    rng = np.random.default_rng(42)
    buf = filler(rng, 1_200_000, lo=32)
    pl = Cells(rng, buf)
    pl.put([20, 21], 290)
    pl.put([0, 1, 3], 260)
    pl.put([0, 1], 20)
    for i in range(6):
        pl.put([4 + 2 * i, 5 + 2 * i], 250 - 10 * i)
    return [buf, filler(rng, 555, lo=32)], [1] * HOT_BASE


@gpu
def test_a_merge_of_the_new_id_scans_and_the_lists_serve_the_rest(monkeypatch):
    monkeypatch.delenv('BPE_DIGEST_CAND', raising=False)
    samples, len16 = miss_corpus()
    c = HOT_BASE + 1
    wanted = {(20, 21), (0, 1), (c, 3)} | {(4 + 2 * i, 5 + 2 * i) for i in range(5)}
    stats, merges, per_batch = drive(samples, len16, 0, 1, wanted)
    print(per_batch)
    assert merges[:4] == [(20, 21, 290), (0, 1, 280), (c, 3, 260), (4, 5, 250)], merges
    assert stats['digest_passes'] == 8, stats
    if K > 1:
        # no scan can have answered for (c, 3): c did not exist when the one before it ran
        assert 2 <= stats['digest_scans'] < 8, stats
    if K == 4:
        # (20, 21) with (0, 1), (4, 5), (6, 7); the miss (c, 3) with (4, 5), (6, 7), (8, 9); three
        # merges from those lists; (10, 11) with (12, 13)
        assert stats['digest_scans'] == 3, stats


# ---- (d) edge sites from a cached list -------------------------------------------------------------
def edge_corpus():
    """(0, 1), W 200: every site has its 0 in slot 255 and its 1 in slot 0 of the next chunk, at
    chunk boundaries of both parities (inside a region and across two).  The chunk of each 0 also
    holds a site of (2, 3), W 260, which merges before it: the 0 is then still its chunk's last
    live token, before a dead slot and the tail tag.  (4, 5), W 290, goes first; five lighter
    pairs follow."""
    rng = np.random.default_rng(43)
    buf = filler(rng, 1_200_000)
    for k in range(100, 300):
        buf[CHUNK * k - 1:CHUNK * k + 1] = [0, 1]
        buf[CHUNK * k - 120:CHUNK * k - 118] = [2, 3]
    pl = Cells(rng, buf)
    pl.cells = iter([c for c in pl.cells if not 90 * 4 <= c <= 310 * 4])
    pl.edges = iter([c for c in pl.edges if not 90 <= c <= 310])
    pl.put([2, 3], 60)
    pl.put([4, 5], 290)
    for i in range(5):
        pl.put([6 + 2 * i, 7 + 2 * i], 180 - 10 * i)
    return [buf, filler(rng, 555)], [1] * HOT_BASE


@gpu
def test_edge_sites_in_chunks_an_earlier_listed_merge_shortened(monkeypatch):
    monkeypatch.delenv('BPE_DIGEST_CAND', raising=False)
    samples, len16 = edge_corpus()
    wanted = {(4, 5), (2, 3), (0, 1)} | {(6 + 2 * i, 7 + 2 * i) for i in range(5)}
    stats, merges, per_batch = drive(samples, len16, 0, 1, wanted)
    print(per_batch)
    assert merges[:3] == [(4, 5, 290), (2, 3, 260), (0, 1, 200)], merges
    assert stats['digest_passes'] == 8, stats
    if K > 2:
        # (2, 3) and (0, 1) are read by the scan for (4, 5)
        assert stats['digest_scans'] <= 8 - 2, stats
    if K == 4:
        # (4, 5) scans for itself, (2, 3), (0, 1) and (6, 7), which are applied from those rows;
        # (8, 9) scans for itself and the last three
        assert stats['digest_scans'] == 2, stats


# ---- (e) compaction ---------------------------------------------------------------------------------
@gpu
def test_compaction_drops_the_lists_and_the_next_batch_scans_again(monkeypatch):
    """A heavy merge first (the full form: the plane and the lists are dropped on the device, the
    next call compacts); the second batch builds the plane of the new layout and scans it."""
    monkeypatch.delenv('BPE_DIGEST_CAND', raising=False)
    samples, len16 = light_pairs_corpus(16, heavy=13_000)
    wanted = {(2 * i, 2 * i + 1) for i in range(15)}
    stats, merges, per_batch = drive(samples, len16, 0, 2, wanted)
    print(per_batch)
    b0, b1 = per_batch[0], per_batch[1]
    assert b0['digest_passes'] == 0 and b0['digest_scans'] == 0 and b0['delta_passes'] == 7, b0
    assert b1['compactions'] == 1 and b1['digest_builds'] == 2, b1
    assert b1['digest_passes'] == 8 and b1['digest_scans'] >= 1, b1
    if K > 1:
        assert b1['digest_scans'] < 8, b1


# ---- (f) geometry -----------------------------------------------------------------------------------
@gpu
def test_rows_of_two_words_and_sites_at_region_edges(monkeypatch):
    """36 M tokens: 140 626 chunks, 35 per region, so a row is two words, the second with three
    bits in use, and a region's chunks are no multiple of the four of a wave-load.  The background
    of 168 hot ids counts about 1300 per pair here, so the eight light pairs weigh 8000 - 500 i
    (16 W below the chunks): of each, 25 sites across the boundary before a region's first chunk,
    25 inside a region's first chunk, 25 inside its last (word 1, bit 2) and 25 inside its chunk
    32 (word 1, bit 0), each in a region of its own among the first 1000; the rest anywhere in
    the other regions, every third across a chunk boundary."""
    monkeypatch.delenv('BPE_DIGEST_CAND', raising=False)
    rng = np.random.default_rng(44)
    n = 36_000_000
    buf = filler(rng, n, lo=32)
    nch = (n + 1 + CHUNK - 1) // CHUNK
    cpr = -(-nch // 4096)
    assert cpr == 35 and nch % 4 != 0 and cpr % 4 != 0 and 16 * 8000 < nch
    regions = iter(rng.permutation(np.arange(2, 1000)))
    pl = Placer(rng, buf[CHUNK * cpr * 1002:])
    for i in range(8):
        x, y = 2 * i, 2 * i + 1
        for j in range(100):
            c0 = int(next(regions)) * cpr
            pos = CHUNK * (c0 + (0, 0, cpr - 1, 32)[j % 4]) + (0 if j % 4 == 0 else 10 + j)
            buf[pos - 1:pos + 1] = [x, y]
        pl.pair(x, y, 8000 - 500 * i - 100, every=3)
    len16 = [1] * HOT_BASE
    st = OracleState(buf, np.array([0, n], np.int64), len16, len(len16), extra=64)
    want = st.merge_until(0, 2, 8)
    assert want == [(2 * i, 2 * i + 1, 8000 - 500 * i) for i in range(8)], want
    e = make_engine([buf], len16)
    e.stats_enable(True)
    try:
        assert e.merge_until(0, 2, 8) == want
        check_table(e)
        stats = e.stats()
        print(stats)
        ids, off = e.read_corpus()
        assert off.tolist() == [0, len(st.ids)] and np.array_equal(ids, st.ids)
        assert stats['digest_passes'] == 8 and stats['delta_passes'] == 8, stats
        if K > 1:
            # some merges from a scan, some from a list
            assert 0 < stats['digest_scans'] < 8, stats
    finally:
        e.close()
