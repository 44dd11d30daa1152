"""The digest plane of the device loop's delta form: one byte per corpus slot (pkg.digest), through
which a delta iteration's stream finds the few chunks that can hold a site of the merge; only
those chunks' int32 slots are loaded and take the exact path of the int32 stream.  Every GPU test
drives mergeUntil in batches of 8 merges and requires, after every batch, the merges and the
samples of the oracle and a maintained table equal to a recount in all 81 920 bins; the corpora
keep the pairs meant for the delta form below 1/16 of their chunks (checked against the oracle's W
before anything is asserted about the engine).  Sizes: 1 - 3 M tokens, three chunks per region."""
import ctypes
import functools

import numpy as np
import pytest

from bpe_amd import make_engine, pkg
from oracle import OracleState

gpu = pytest.mark.gpu

CHUNK = 256
HOT_BASE = 200      # base ids of the placed corpora: the merged tokens stay hot
FILL_LO = 16        # ids below it are kept for the placed structures


def _hip():
    """The HIP runtime libbpe runs on (the engine's device buffers belong to it)."""
    pkg.lib()
    with open('/proc/self/maps') as f:
        rts = sorted({ln.split()[-1] for ln in f if 'libamdhip64' in ln and '/' in ln})
    own = [p for p in rts if 'torch' not in p] or rts
    h = ctypes.CDLL(own[0] if own else 'libamdhip64.so')
    h.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    h.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    h.hipFree.argtypes = [ctypes.c_void_p]
    return h


def table_of(e):
    """The engine's [TABLE_BINS] u64 pair table (hot bins + sketch buckets) on the host."""
    h = _hip()
    n = pkg.TABLE_BINS
    p = ctypes.c_void_p()
    assert h.hipMalloc(ctypes.byref(p), 8 * n) == 0
    try:
        e.export_counts(p.value)
        out = np.zeros(n, np.uint64)
        assert h.hipMemcpy(out.ctypes.data, p, 8 * n, 2) == 0   # hipMemcpyDeviceToHost
    finally:
        h.hipFree(p)
    return out


def filler(rng, n, lo=FILL_LO):
    """A near-unique background of the hot ids lo .. HOT_BASE - 1."""
    return rng.integers(lo, HOT_BASE, size=n).astype(np.int32)


class Placer:
    """Puts two-token structures into buf so that none touches another: `inside` at offsets
    2 .. 61 of a 64-token cell of its own, `across` with its first token in slot 255 of a chunk
    of its own and its second in slot 0 of the next."""

    def __init__(self, rng, buf):
        self.rng, self.buf = rng, buf
        self.cells = iter(rng.permutation(np.arange(8, len(buf) // 64 - 8)))
        self.edges = iter(rng.permutation(np.arange(4, len(buf) // CHUNK - 4)))

    def inside(self, x, y):
        pos = int(next(self.cells)) * 64 + int(self.rng.integers(2, 60))
        self.buf[pos:pos + 2] = [x, y]

    def across(self, x, y):
        pos = int(next(self.edges)) * CHUNK
        self.buf[pos - 1:pos + 1] = [x, y]

    def pair(self, x, y, count, every=0):
        """count sites of (x, y), every `every`-th across a chunk boundary."""
        for i in range(count):
            if every and i % every == 0:
                self.across(x, y)
            else:
                self.inside(x, y)


def flat(samples):
    off = np.concatenate([[0], np.cumsum([len(s) for s in samples])]).astype(np.int64)
    return np.concatenate(samples).astype(np.int32), off


def n_chunks_of(samples):
    """Chunks of the packed corpus: every sample is its tokens and one separator."""
    return (sum(len(s) + 1 for s in samples) + CHUNK - 1) // CHUNK


def check_table(e):
    kept = table_of(e)
    e.recount()
    fresh = table_of(e)
    bad = np.nonzero(kept != fresh)[0]
    assert bad.size == 0, [(int(i), int(kept[i]), int(fresh[i])) for i in bad[:8]]


def drive(samples, len16, max_length, batches, want_delta, between=None):
    """mergeUntil in `batches` batches of 8 against the oracle; after every batch the merges, the
    samples and table == recount.  want_delta: ids (a, b) the oracle must merge with
    16 W < chunks (the corpus check), and the engine must then report delta passes.
    between(e, st, want): called after every batch but the last (it may merge on both sides).
    Returns the final stats, the merges and the stats after every batch."""
    ids, off = flat(samples)
    st = OracleState(ids, off, len16, len(len16), extra=1024)
    want = []
    nch = n_chunks_of(samples)
    e = make_engine(samples, len16)
    e.stats_enable(True)
    seen = set()
    per_batch = []
    try:
        for i in range(batches):
            w = st.merge_until(max_length, 2, 8)
            for a, b, W in w:
                if (a, b) in want_delta:
                    assert a != b and 16 * W < nch, ('corpus: not a delta merge', a, b, W, nch)
                    seen.add((a, b))
            got = e.merge_until(max_length, 2, 8)
            assert got == w
            want += w
            check_table(e)
            per_batch.append(e.stats())
            if len(w) < 8:
                break
            if between is not None and i + 1 < batches:
                between(e, st, want)
        assert seen == set(want_delta), ('corpus: merges not reached', set(want_delta) - seen)
        assert e.samples() == st.samples()
        return e.stats(), want, per_batch
    finally:
        e.close()


# ---- 6. the exported digest (no GPU) -------------------------------------------------------------
def test_exported_digest_matches_its_restatement():
    ids = np.array([-1, -2, -4, -3, -16, -16 - 255 - ((55295 + 3) << 8), 0, 1, 253, 254, 255, 256,
                    507, 508, 509, 55295], np.int32)
    want = np.where(ids >= 0, ids % pkg.DIGEST_MOD,
                    np.where(ids == -1, pkg.DIGEST_SEP, pkg.DIGEST_DEAD)).astype(np.uint8)
    assert pkg.digest(ids).tolist() == want.tolist()
    # separator and dead codes are distinct from each other and from every token's digest
    assert pkg.DIGEST_SEP != pkg.DIGEST_DEAD and min(pkg.DIGEST_SEP, pkg.DIGEST_DEAD) >= pkg.DIGEST_MOD
    assert max(pkg.DIGEST_SEP, pkg.DIGEST_DEAD) <= 255
    assert int(pkg.digest(np.arange(55296, dtype=np.int32)).max()) == pkg.DIGEST_MOD - 1


# ---- 1. aliases, and 5. the knob -----------------------------------------------------------------
def alias_ids():
    """Hot ids a != a2 and b != b2 with digest(a) == digest(a2) and digest(b) == digest(b2), found
    from the exported function."""
    d = pkg.digest(np.arange(256, dtype=np.int32))
    for a in range(FILL_LO):
        for b in range(a + 1, FILL_LO):
            a2 = [t for t in range(HOT_BASE, 256) if d[t] == d[a]]
            b2 = [t for t in range(HOT_BASE, 256) if d[t] == d[b]]
            if a2 and b2 and a2[0] != b2[0]:
                return a, b, a2[0], b2[0]
    raise AssertionError('no aliasing hot ids: the alias test needs another pair')


def alias_corpus():
    """1.2 M tokens (4688 chunks): 250 true (a, b) sites among the decoys (a2, b2) x 280,
    (a2, b) x 260, (a, b2) x 230 and 40 more (a, b2) with a last in its chunk and b2 first in the
    next: every one of the four pairs is a delta merge, and the other three are its decoys."""
    a, b, a2, b2 = alias_ids()
    rng = np.random.default_rng(21)
    buf = filler(rng, 1_200_000)
    pl = Placer(rng, buf)
    for x, y, cnt in ((a, b, 250), (a2, b2, 280), (a2, b, 260), (a, b2, 230)):
        pl.pair(x, y, cnt, every=5)
    for i in range(40):
        pl.across(a, b2)
    return [buf, filler(rng, 777)], [1] * 256, {(a, b), (a2, b2), (a2, b), (a, b2)}


@functools.lru_cache(maxsize=None)
def alias_run(digest_on):
    """The alias corpus driven with the plane (True) or with BPE_DIGEST=0 (False): run once, shared
    by the tests below (the caller sets the environment)."""
    samples, len16, wanted = alias_corpus()
    return drive(samples, len16, 0, 2, wanted)[:2]


@gpu
def test_aliases_hit_but_only_true_sites_are_rewritten(monkeypatch):
    monkeypatch.delenv('BPE_DIGEST', raising=False)
    stats, merges = alias_run(True)
    monkeypatch.setenv('BPE_DIGEST', '0')
    plain, merges0 = alias_run(False)
    print(stats, plain)
    assert stats['digest_passes'] >= 4, stats
    # the decoys reach the exact path, and only the true sites' chunks are listed
    assert stats['digest_hits'] > stats['delta_chunks'], stats
    assert stats['delta_chunks'] == plain['delta_chunks'], (stats, plain)


@gpu
def test_knob_keeps_the_int32_stream_and_the_results(monkeypatch):
    monkeypatch.delenv('BPE_DIGEST', raising=False)
    stats, merges = alias_run(True)
    monkeypatch.setenv('BPE_DIGEST', '0')
    plain, merges0 = alias_run(False)
    assert merges == merges0
    for key in ('delta_passes', 'delta_chunks', 'tie_passes', 'loop_host'):
        assert stats[key] == plain[key], (key, stats, plain)
    assert plain['digest_passes'] == 0 and plain['digest_hits'] == 0 and plain['digest_builds'] == 0, plain
    assert stats['digest_passes'] > 0 and stats['digest_builds'] >= 1, stats


# ---- 2. edges ------------------------------------------------------------------------------------
def placed_runs_corpus():
    """Placed sites on the filler background, 2.8 M tokens (3 chunks per region), max_length 4, no
    X X pair above them, so that all five merge on the plane in the first batch:
    (0, 1)  a in slot 255 and b in slot 0 of the next chunk, inside a region and across regions,
            every fourth with an a before it (W 526 with the 26 below);
    (7, 8)  chains a b a b .. of 2, 3 and 5 sites across chunk boundaries (W 325);
    (2, 3)  a a .. a b with 600 and 601 a's (3 chunks) and with 0 .. 5 (W 270); len16[2] = 3 keeps
            (2, 2) itself out of the selection;
    (4, 5)  a b b .. b with 600 and 601 b's and with 1 .. 6 (W 200); len16[5] = 3;
    (10, 11) first and last in its sample, alone in its sample, and behind a chunk the (0, 1)
            merge left partial (W 171);
    and, not a site: 10 as the last live token of a chunk the (0, 1) merge left partial, the next
    chunk starting with a separator and then 11 (six sample boundaries at chunk boundaries)."""
    rng = np.random.default_rng(11)
    n = CHUNK * 10937        # (the sample's separator is slot 0 of the next chunk)
    buf = filler(rng, n)

    def put(pos, toks):
        buf[pos:pos + len(toks)] = toks

    # (7, 8): 5 * 2 + 5 * 3 + 60 * 5 sites
    for i in range(5):
        put(CHUNK * (60 + 2 * i) - 1 - i, [7, 8] * 2)
        put(CHUNK * (80 + 2 * i) - 2 - i, [7, 8] * 3)
    for i in range(60):
        put(CHUNK * (2100 + 2 * i) - 1 - i % 9, [7, 8] * 5)
    # (0, 1): 500 chunk boundaries (3 chunks per region: both kinds)
    for k in range(100, 600):
        put(CHUNK * k - 1, [0, 1])
        if k % 4 == 0:
            put(CHUNK * k - 2, [0])
    # (2, 3): runs of a
    put(CHUNK * 1000 - 100, [2] * 600 + [3])
    put(CHUNK * 1010 - 100, [2] * 601 + [3])
    for i in range(268):
        put(CHUNK * 1100 + 50 * i, [2] * (1 + i % 6) + [3])
    # (4, 5): runs of b
    put(CHUNK * 1300 - 100, [4] + [5] * 600)
    put(CHUNK * 1310 - 100, [4] + [5] * 601)
    for i in range(198):
        put(CHUNK * 1400 + 50 * i, [4] + [5] * (1 + i % 6))
    # (10, 11) behind a chunk left partial: .. 0 1 10 | 11 ..
    for k in range(2000, 2020):
        put(CHUNK * k - 3, [0, 1, 10, 11])
    # .. 0 1 10 | SEP 11 ..: the sample ends at the chunk's end
    put(n - 3, [0, 1, 10])
    samples = [buf]
    for i in range(5):
        s = filler(rng, CHUNK * 3 - 1)
        s[0] = 11
        s[-3:] = [0, 1, 10]
        samples.append(s)
    tail = filler(rng, 400)
    tail[0] = 11
    samples.append(tail)
    # (10, 11) first and last in a sample, and alone in one
    for i in range(75):
        samples.append(np.concatenate([[10, 11], filler(rng, 17), [10, 11]]).astype(np.int32))
    samples.append(np.array([10, 11], np.int32))
    len16 = [1] * HOT_BASE
    len16[2] = len16[5] = 3
    return samples, len16


@gpu
def test_placed_runs_chains_and_boundaries():
    samples, len16 = placed_runs_corpus()
    assert n_chunks_of(samples[:1]) == 10938 and len(samples[0]) % CHUNK == 0
    wanted = {(7, 8), (0, 1), (2, 3), (4, 5), (10, 11)}
    stats, merges, per_batch = drive(samples, len16, 4, 2, wanted)
    print(per_batch)
    assert merges[:5] == [(0, 1, 526), (7, 8, 325), (2, 3, 270), (4, 5, 200), (10, 11, 171)], merges[:5]
    # (the separated 10 | SEP 11 are hits and no sites: W stays 171)
    assert per_batch[0]['digest_passes'] >= len(wanted), per_batch[0]
    assert per_batch[0]['digest_hits'] > 0, per_batch[0]


def placed_empties_corpus():
    """130 sections of two chunks of 12 13 12 13 .., each behind a chunk ending in 14 and before a
    chunk starting with 15: eight heavy merges (full passes) leave one token z in each chunk of
    a section; then (14, z), (z, z) and (z, 15) tie at W 130 (the tie pass).  (14, z) -> u goes
    first and empties the section's first chunk (its site lies across two chunks); (z, 15) -> v
    then has its left neighbour u beyond that emptied chunk, and (u, v) -> w is a site whose two
    halves lie either side of it and which empties the section's second chunk too.  420 (0, 1)
    sites across chunk boundaries merge in the delta form between the heavy ones.  Those merges
    meet a stale plane (the heavy ones before them); four light pairs (W 125 .. 110) fill the
    second batch, and the third, on a rebuilt plane, begins with (w, 9): in 100 sections a 9
    follows the 15, so w is its chunk's last live token and the 9 lies beyond two empty chunks."""
    rng = np.random.default_rng(12)
    n = 1_800_000
    buf = filler(rng, n)
    for s in range(130):
        c0 = 50 + 40 * s
        buf[CHUNK * c0:CHUNK * (c0 + 2)] = [12, 13] * CHUNK
        buf[CHUNK * c0 - 1] = 14
        buf[CHUNK * (c0 + 2)] = 15
        if s < 100:
            buf[CHUNK * (c0 + 2) + 1] = 9
    for k in range(5500, 5920):
        buf[CHUNK * k - 1] = 0
        buf[CHUNK * k] = 1
    pos = CHUNK * 6000
    for x, y, cnt in ((2, 3, 125), (4, 5, 120), (6, 7, 115), (8, 10, 110)):
        for _ in range(cnt):
            buf[pos:pos + 2] = [x, y]
            pos += 97
    return [buf, filler(rng, 999)], [1] * HOT_BASE


@gpu
def test_placed_sites_beyond_emptied_chunks():
    samples, len16 = placed_empties_corpus()
    stats, merges, per_batch = drive(samples, len16, 0, 3, {(0, 1)})
    print(per_batch)
    assert stats['delta_passes'] >= 4, stats
    tail = [m for m in merges if m[2] == 130]
    assert len(tail) == 3 and tail[0][0] == 14 and tail[1][1] == 15, merges
    w = HOT_BASE + merges.index(tail[2])
    assert tail[2][:2] == (HOT_BASE + merges.index(tail[0]), HOT_BASE + merges.index(tail[1]))
    assert [m[:2] for m in merges[12:16]] == [(2, 3), (4, 5), (6, 7), (8, 10)], merges[12:16]
    assert merges[16] == (w, 9, 100), merges[16]
    # the third batch runs on a rebuilt plane
    assert per_batch[2]['digest_builds'] == 2, per_batch
    assert per_batch[2]['digest_passes'] > per_batch[1]['digest_passes'], per_batch


# ---- 3. and 4. staleness -------------------------------------------------------------------------
XX = 30             # the staleness corpora's X X pair, and their heavy pair
HEAVY = (29, 28)


def light_pairs_corpus(n_pairs, xx_at=None, heavy=None):
    """1.2 M tokens (4690 chunks) over the filler ids 32 .. 199: light pairs (2 i, 2 i + 1),
    i < n_pairs, with W = 280 - 6 i exactly (every third site across a chunk boundary); xx_at: an
    X X pair (30, 30) whose W falls after that many light pairs; heavy: W of the pair (29, 28),
    in at least 1/16 of the chunks (a full-form merge)."""
    rng = np.random.default_rng(31)
    buf = filler(rng, 1_200_000, lo=32)
    pl = Placer(rng, buf)
    for i in range(n_pairs):
        pl.pair(2 * i, 2 * i + 1, 280 - 6 * i, every=3)
    if xx_at is not None:
        pl.pair(XX, XX, 280 - 6 * xx_at + 3)
    if heavy:
        pl.pair(HEAVY[0], HEAVY[1], heavy)
    return [buf, filler(rng, 555, lo=32)], [1] * HOT_BASE


@gpu
def test_plane_goes_stale_inside_a_batch_and_is_rebuilt():
    """Two light merges, an X X merge (the full pass: the plane is stale), five light ones on the
    int32 stream; the next batch rebuilds the plane."""
    samples, len16 = light_pairs_corpus(7, xx_at=2)
    wanted = {(2 * i, 2 * i + 1) for i in range(7)}
    stats, merges, per_batch = drive(samples, len16, 0, 2, wanted)
    print(per_batch)
    assert [m[:2] for m in merges[:4]] == [(0, 1), (2, 3), (XX, XX), (4, 5)], merges[:4]
    b0, b1 = per_batch[0], per_batch[1]
    assert b0['digest_passes'] == 2 and b0['delta_passes'] == 7, b0
    assert b0['delta_passes'] - b0['digest_passes'] > 0
    assert b1['digest_passes'] > b0['digest_passes'], (b0, b1)
    assert b1['digest_builds'] >= 2, b1


@gpu
def test_host_path_merge_between_batches_makes_the_plane_stale():
    samples, len16 = light_pairs_corpus(10)
    wanted = {(2 * i, 2 * i + 1) for i in range(7)}

    def one_host_merge(e, st, want):
        w = st.merge_until(0, 2, 1)
        a, b, W = e.find_next_merge(0, 2)
        assert [(a, b, W)] == w
        assert e.apply_merge(a, b, HOT_BASE + len(want)) == W
        want += w

    stats, merges, per_batch = drive(samples, len16, 0, 2, wanted, between=one_host_merge)
    print(per_batch)
    assert merges[8][:2] == (16, 17), merges[8]
    b0, b1 = per_batch[0], per_batch[1]
    assert b0['digest_passes'] == 8 and b0['digest_builds'] == 1, b0
    assert b1['digest_builds'] == 2 and b1['digest_passes'] > 8, b1


def stale_between(between):
    """A batch of eight light merges on a fresh plane, one merge by `between` (a writer of the
    corpus outside the device loop), a second batch: it rebuilds the plane and reads it again."""
    samples, len16 = light_pairs_corpus(10)
    wanted = {(2 * i, 2 * i + 1) for i in range(7)}
    stats, merges, per_batch = drive(samples, len16, 0, 2, wanted, between=between)
    print(per_batch)
    assert merges[8][:2] == (16, 17), merges[8]
    b0, b1 = per_batch[0], per_batch[1]
    assert b0['digest_passes'] == 8 and b0['digest_builds'] == 1, b0
    assert b1['digest_builds'] == 2 and b1['digest_passes'] > 8, b1


@gpu
@pytest.mark.parametrize('count_after', [False, True], ids=['apply_only', 'counting'])
def test_replay_between_batches_makes_the_plane_stale(count_after):
    """apply_merges of one merge: the apply-only pass (k_apply), or with count_after the counting
    pass of the host path."""
    def one_replayed_merge(e, st, want):
        w = st.merge_until(0, 2, 1)
        (a, b, W), = w
        got = e.apply_merges([(a, b, HOT_BASE + len(want))], count_after=count_after)
        assert [int(r) for r in got] == [W]
        want += w

    stale_between(one_replayed_merge)


@gpu
def test_position_index_merge_between_batches_makes_the_plane_stale():
    """One merge in the incremental mode: the index merges in place in the corpus buffer, and the
    corpus is written back to the chunk layout."""
    def one_index_merge(e, st, want):
        w = st.merge_until(0, 2, 1)
        e.set_mode('incremental')
        assert e.merge_until(0, 2, 1) == w
        e.set_mode('stream')
        want += w

    stale_between(one_index_merge)


@gpu
def test_compaction_between_batches_makes_the_plane_stale():
    """A heavy merge first (the full form: 1 % of the slots die, so the next call compacts), seven
    light ones on the int32 stream; the next batch runs on a rebuilt plane of the new layout."""
    samples, len16 = light_pairs_corpus(8, heavy=13_000)
    wanted = {(2 * i, 2 * i + 1) for i in range(7)}
    stats, merges, per_batch = drive(samples, len16, 0, 2, wanted)
    print(per_batch)
    assert merges[0] == HEAVY + (13_000,), merges[0]
    b0, b1 = per_batch[0], per_batch[1]
    assert b0['digest_passes'] == 0 and b0['delta_passes'] == 7 and b0['compactions'] == 0, b0
    assert b1['compactions'] == 1 and b1['digest_builds'] == 2 and b1['digest_passes'] >= 1, b1
