"""Plain sites of the delta form: the apply-only stream adds the table deltas of every site whose
two neighbours lie in its own chunk and start no run or chain (x not in {a, c}, y not in {b, c}),
and lists for the site walk only the chunks holding another kind of site.  `delta_chunks` counts
the chunks a delta iteration rewrote, `site_chunks` those of them it listed.

Every test drives mergeUntil in batches of 8 against the oracle as test_delta_pass does (merges,
samples, and the kept table equal to a recount in all bins after every batch), and compares the two
statistics with a model of the chunk layout written from the definition alone (ChunkModel: chunks
are left-packed and no merge moves a token to another chunk).  The corpora are checked against the
oracle's W first, so no test passes by never reaching the delta form."""
import numpy as np
import pytest

from bpe_amd import make_engine
from oracle import OracleState
from test_delta_pass import BASE, CHUNK, HOT_BASE, filler, flat, n_chunks_of, table_of

pytestmark = pytest.mark.gpu

N = 600_000          # tokens of the small corpora: 2344 chunks, one chunk per region
N_EDGES = 1_100_000  # the edges corpus: 4297 chunks, two per region (both kinds of chunk boundary)


class ChunkModel:
    """The live slots of the packed corpus (tokens and one -1 after every sample) with the chunk
    each sits in.  merge() applies (a, b) -> c and returns (replacements, chunks rewritten, chunks
    holding a site that is not plain)."""

    def __init__(self, samples):
        self.tok = np.concatenate([np.append(np.asarray(s, np.int64), -1) for s in samples])
        self.chunk = np.arange(self.tok.size) // CHUNK

    def merge(self, a, b, c):
        t = self.tok
        i = np.nonzero((t[:-1] == a) & (t[1:] == b))[0]
        if a == b:   # leftmost non-overlapping occurrences
            take, last = [], -2
            for p in i.tolist():
                if p != last + 1:
                    take.append(p)
                    last = p
            i = np.asarray(take, np.int64)
        rewritten = np.union1d(self.chunk[i], self.chunk[i + 1])
        t[i] = c
        keep = np.ones(t.size, bool)
        keep[i + 1] = False
        self.tok, self.chunk = t[keep], self.chunk[keep]
        t = self.tok
        j = np.nonzero(t == c)[0]
        ch = self.chunk[j]
        k = j - np.searchsorted(self.chunk, ch, 'left')
        ln = np.searchsorted(self.chunk, ch, 'right') - np.searchsorted(self.chunk, ch, 'left')
        x = np.where(j > 0, t[np.maximum(j - 1, 0)], -1)
        y = t[j + 1]   # (the corpus ends in a separator)
        plain = (k > 0) & (k < ln - 1) & (x != a) & (x != c) & (y != b) & (y != c)
        return i.size, rewritten.size, np.unique(ch[~plain]).size, int(plain.sum())


def samples_of(slots):
    """The samples of a slot array in which -1 ends a sample (the last slot is one)."""
    slots = np.asarray(slots, np.int32)
    ends = np.nonzero(slots == -1)[0]
    assert ends.size and ends[-1] == slots.size - 1 and (np.diff(ends) > 1).all() and ends[0] > 0
    return [s[:-1] for s in np.split(slots, ends + 1)[:-1]]


def run(samples, n_base, batches, want_delta, max_length=0):
    """test_delta_pass.drive, and with it the model: returns the statistics, the merges, the kept
    table after the last batch and per merge (a, b, W, delta form expected, rewritten, listed,
    plain sites).  Asserts delta_passes, delta_chunks and site_chunks equal to the model's."""
    len16 = [1] * n_base
    ids, off = flat(samples)
    st = OracleState(ids, off, len16, n_base, extra=1024)
    model = ChunkModel(samples)
    nch = n_chunks_of(samples)
    rows, merges, seen = [], [], set()
    e = make_engine(samples, len16)
    e.stats_enable(True)
    try:
        for _ in range(batches):
            w = st.merge_until(max_length, 2, 8)
            for a, b, W in w:
                if (a, b) in want_delta:
                    assert a != b and 16 * W < nch, ('corpus: not a delta merge', a, b, W, nch)
                    seen.add((a, b))
            got = e.merge_until(max_length, 2, 8)
            assert got == w
            for a, b, W in w:
                n, rewritten, listed, plain = model.merge(a, b, n_base + len(merges))
                assert n == W, ('model', a, b, W, n)
                rows.append((a, b, W, a != b and 16 * W < nch, rewritten, listed, plain))
                merges.append((a, b, W))
            kept = table_of(e)
            e.recount()
            fresh = table_of(e)
            bad = np.nonzero(kept != fresh)[0]
            assert bad.size == 0, [(int(i), int(kept[i]), int(fresh[i])) for i in bad[:8]]
            if len(w) < 8:
                break
        assert seen == set(want_delta), ('corpus: merges not reached', set(want_delta) - seen)
        assert e.samples() == st.samples()
        stats = e.stats()
    finally:
        e.close()
    print(stats)
    print(rows)
    delta = [r for r in rows if r[3]]
    assert stats['loop_host'] == 0, stats
    assert stats['delta_passes'] == len(delta), (stats, rows)
    assert stats['delta_chunks'] == sum(r[4] for r in delta), (stats, rows)
    assert stats['site_chunks'] == sum(r[5] for r in delta), (stats, rows)
    return stats, merges, kept, rows


# ---- 1. only plain sites ---------------------------------------------------------------------
PAIRS8 = [(2 * j, 2 * j + 1) for j in range(8)]


def plain_corpus(base):
    """Eight pairs (0, 1) .. (14, 15), W 140, 135 .. 105, every site alone in a chunk of its own
    at a slot in 1 .. 253, between filler ids: the eight merges of one batch."""
    rng = np.random.default_rng(21)
    buf = filler(rng, N, base)
    t = 0
    for j, (a, b) in enumerate(PAIRS8):
        for _ in range(140 - 5 * j):
            p = CHUNK * (2 * t + 1) + int(rng.integers(1, 254))
            buf[p:p + 2] = [a, b]
            t += 1
    assert CHUNK * (2 * t + 1) < N
    return [buf]


@pytest.mark.parametrize('base', [HOT_BASE, BASE])
def test_only_plain_sites_list_nothing(base):
    stats, merges, _, rows = run(plain_corpus(base), base, 1, set(PAIRS8))
    assert [m[:2] for m in merges] == PAIRS8, merges
    assert stats['delta_passes'] == 8 and stats['delta_chunks'] == sum(m[2] for m in merges), stats
    assert stats['site_chunks'] == 0, stats


# ---- 2. edges --------------------------------------------------------------------------------
def edges_corpus():
    """(0, 1) W 250: sites in slot 0.  (2, 3) W 240: sites in the last live slot (slots 254, 255).
    (4, 5) W 230: a in slot 255, b in slot 0 of the next chunk, half of them inside a region and
    half across two regions (two chunks per region).  (6, 7) W 220: a sample ends behind the site,
    or begins with it, mid-chunk; and one in ten of those in slot 0 behind a separator in slot 255.
    (8, 9) W 210: first in the corpus, last in the corpus, the others mid-chunk.  Returns the
    samples and, per pair, the chunks the model must find listed."""
    rng = np.random.default_rng(22)
    s = filler(rng, N_EDGES, HOT_BASE)
    s[-1] = -1
    want = {}
    for k in range(250):
        s[CHUNK * (10 + k):CHUNK * (10 + k) + 2] = [0, 1]
    want[(0, 1)] = 250
    for k in range(240):
        s[CHUNK * (300 + k) + 254:CHUNK * (300 + k) + 256] = [2, 3]
    want[(2, 3)] = 240
    for k in range(230):
        q = 600 + 3 * k   # boundary q | q + 1: odd q ends a region, even q does not
        s[CHUNK * q + 255:CHUNK * q + 257] = [4, 5]
    want[(4, 5)] = 230
    listed = 0
    for k in range(220):
        p = CHUNK * (1400 + 2 * k)
        if k % 10 == 0:
            s[p - 1:p + 2] = [-1, 6, 7]          # slot 0, behind a separator in another chunk
            listed += 1
        elif k & 1:
            s[p + 99:p + 102] = [6, 7, -1]       # x a b SEP
        else:
            s[p + 99:p + 102] = [-1, 6, 7]       # SEP a b y
    want[(6, 7)] = listed
    s[0:2] = [8, 9]
    s[-3:-1] = [8, 9]
    for k in range(208):
        p = CHUNK * (2000 + 2 * k) + 77
        s[p:p + 2] = [8, 9]
    want[(8, 9)] = 1   # (the last one sits before the corpus's final separator: plain)
    return samples_of(s), want


def test_edge_sites_are_listed_and_only_they():
    samples, want = edges_corpus()
    assert n_chunks_of(samples) > 4096 + 200   # (two chunks per region)
    stats, merges, _, rows = run(samples, HOT_BASE, 1, set(want))
    assert [m[:2] for m in merges[:5]] == list(want), merges
    for r in rows[:5]:
        assert r[5] == want[r[:2]], (r, want)
    # (the boundary sites rewrite two chunks each and list one)
    assert rows[2][4] == 2 * 230 and rows[2][6] == 0, rows[2]
    # (the separators' sites are plain but for those in slot 0)
    assert rows[3][6] == 220 - want[(6, 7)] and rows[4][6] == 209, rows[3:5]


# ---- 3. / 4. mixed chunks --------------------------------------------------------------------
def mixed_corpus():
    """Chunks that hold two plain sites (slots 10 and 20) and one structure of another kind:
    (0, 1)  x == a: runs a a b, a a a b, a a a a b at slot 40, and a run that begins in the chunk
            before (its last one or two slots) and ends in a b at slot 0;
    (2, 3)  y == b: a b b, a b b b, a b b b b at slot 40;
    (4, 5)  chains a b a b a b at slot 40, and a b a b at slots 254 .. 257 (across two chunks);
    (6, 7)  a b x a b (c x c: both plain) at slot 40 and a site in slot 0."""
    rng = np.random.default_rng(23)
    buf = filler(rng, N, HOT_BASE)
    q = [3]

    def chunk(a, b, at40, at0=None, before=None):
        p = CHUNK * q[0]
        buf[p + 10:p + 12] = [a, b]
        buf[p + 20:p + 22] = [a, b]
        buf[p + 40:p + 40 + len(at40)] = at40
        if at0:
            buf[p:p + len(at0)] = at0
        if before:
            buf[p - len(before):p] = before
        q[0] += 3

    for i in range(36):
        k = i % 5
        if k < 3:
            chunk(0, 1, [0] * (2 + k) + [1])
        else:
            chunk(0, 1, [0, 1], at0=[0, 1], before=[0] * (k - 2))
    for i in range(40):
        chunk(2, 3, [2] + [3] * (2 + i % 3))
    for i in range(24):
        if i % 3:
            chunk(4, 5, [4, 5] * 3)
        else:
            chunk(4, 5, [4, 5])
            p = CHUNK * (q[0] - 3)
            buf[p + 254:p + 258] = [4, 5, 4, 5]
    for i in range(22):
        chunk(6, 7, [6, 7, 16 + i, 6, 7], at0=[6, 7])
    assert CHUNK * q[0] < N
    return [buf]


MIXED = {(0, 1), (2, 3), (4, 5), (6, 7)}


_mixed = []


def mixed_reference():
    """The mixed corpus under the default settings (the digest stream, four candidate pairs),
    computed once for the tests below."""
    if not _mixed:
        _mixed.append(run(mixed_corpus(), HOT_BASE, 2, MIXED))
    return _mixed[0]


def test_mixed_chunks_count_every_site_once():
    stats, merges, _, rows = mixed_reference()
    by = {r[:2]: r for r in rows}
    # every chunk of a placed pair is listed, and holds plain sites beside the others
    for ab, n in (((0, 1), 36), ((2, 3), 40), ((6, 7), 22)):
        assert by[ab][5] == n and by[ab][6] >= 2 * n, by[ab]
    assert by[(4, 5)][5] == 24 + 8 and by[(4, 5)][6] >= 2 * 24, by[(4, 5)]
    assert 0 < stats['site_chunks'] < stats['delta_chunks'], stats


@pytest.mark.parametrize('env', [{'BPE_DIGEST': '0'}, {'BPE_DIGEST_CAND': '1'},
                                 {'BPE_DIGEST_CAND': '8'}])
def test_mixed_chunks_in_both_bodies_and_from_the_lists(env, monkeypatch):
    plain = mixed_reference()
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    stats, merges, table, _ = run(mixed_corpus(), HOT_BASE, 2, MIXED)
    assert merges == plain[1]
    assert (table == plain[2]).all()
    for key in ('delta_passes', 'delta_chunks', 'site_chunks'):
        assert stats[key] == plain[0][key], (key, stats, plain[0])
    if env.get('BPE_DIGEST') == '0':
        assert stats['digest_passes'] == 0 and plain[0]['digest_passes'] > 0, (stats, plain[0])
    else:
        assert stats['digest_passes'] == plain[0]['digest_passes'] > 0, (stats, plain[0])


# ---- 5. the forms alternating in one launch list ---------------------------------------------
def alternating_corpus():
    """(12, 13) W 150: heavy (16 W >= 2344 chunks), the full pass.  Then delta iterations and X X
    merges in turn: (0, 1) 140, (6, 6) 135, (2, 3) 130, (7, 7) 125, (4, 5) 120, (10, 11) 115,
    (8, 8) 110.  Every third site of the delta pairs lies across a chunk boundary."""
    rng = np.random.default_rng(24)
    buf = filler(rng, N, HOT_BASE)
    order = [((12, 13), 150), ((0, 1), 140), ((6, 6), 135), ((2, 3), 130), ((7, 7), 125),
             ((4, 5), 120), ((10, 11), 115), ((8, 8), 110)]
    t = 0
    for (a, b), W in order:
        for i in range(W):
            p = CHUNK * (2 * t + 1) + (255 if a != b and i % 3 == 0 else int(rng.integers(1, 250)))
            buf[p:p + 2] = [a, b]
            t += 1
    assert CHUNK * (2 * t + 2) < N
    return [buf], order


def test_forms_alternate_in_the_one_launch_list():
    samples, order = alternating_corpus()
    light = {ab for ab, W in order if ab[0] != ab[1] and W < 147}
    stats, merges, _, rows = run(samples, HOT_BASE, 2, light)
    assert merges[:8] == [(a, b, W) for (a, b), W in order], merges[:8]
    assert [r[3] for r in rows[:8]] == [False, True, False, True, False, True, True, False], rows[:8]
    assert stats['delta_passes'] == sum(r[3] for r in rows) >= 4 + 1, (stats, rows)
