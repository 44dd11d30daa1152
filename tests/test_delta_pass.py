"""The delta form of the device loop's table state (LoopCtl::delta): a merge (a, b) -> c of two
distinct ids whose W sites lie in fewer than 1/16 of the chunks is applied by an apply-only stream
that lists the chunks it rewrites, and the pair table is kept by the exact deltas of the sites
(k_site_delta) instead of a recount.  Every test drives mergeUntil in batches of 8 merges and
requires, after every batch, the merges and the samples of the oracle and a maintained table equal
to a recount in all 81 920 bins; the corpora keep the pairs meant for the delta form below 1/16 of
their chunks (checked against the oracle's W before anything is asserted about the engine)."""
import ctypes

import numpy as np
import pytest

from bpe_amd import make_engine, pkg
from oracle import OracleState

pytestmark = pytest.mark.gpu

CHUNK = 256
BASE = 300          # base ids of the random corpora: 256 .. 299 are cold, and so is every merged
                    # token, so their deltas land in sketch buckets
HOT_BASE = 200      # base ids of the placed corpora: the merged tokens stay hot (a cold pair
                    # that wins sends the loop to the host path, then to the maintained state)
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


def filler(rng, n, base=BASE):
    """A near-unique background: ids FILL_LO .. min(base, 256) - 1 and, where base has cold ids,
    2 % of those (so the sketch buckets stay far below the placed pairs' counts)."""
    x = rng.integers(FILL_LO, min(base, 256), size=n).astype(np.int32)
    if base > 256:
        cold = rng.random(n) < 0.02
        x[cold] = rng.integers(256, base, size=int(cold.sum()))
    return x


def flat(samples):
    off = np.concatenate([[0], np.cumsum([len(s) for s in samples])]).astype(np.int64)
    return np.concatenate(samples).astype(np.int32), off


def n_chunks_of(samples):
    """Chunks of the packed corpus: every sample is its tokens and one separator."""
    return (sum(len(s) + 1 for s in samples) + CHUNK - 1) // CHUNK


def drive(samples, len16, max_length, batches, want_delta):
    """mergeUntil in `batches` batches of 8 against the oracle; after every batch the merges, the
    samples and table == recount.  want_delta: ids (a, b) the oracle must merge with
    16 W < chunks (the corpus check), and the engine must then report delta passes."""
    ids, off = flat(samples)
    st = OracleState(ids, off, len16, len(len16), extra=1024)
    want = []
    nch = n_chunks_of(samples)
    e = make_engine(samples, len16)
    e.stats_enable(True)
    seen = set()
    try:
        for _ in range(batches):
            w = st.merge_until(max_length, 2, 8)
            for a, b, W in w:
                if (a, b) in want_delta:
                    assert a != b and 16 * W < nch, ('corpus: not a delta merge', a, b, W, nch)
                    seen.add((a, b))
            got = e.merge_until(max_length, 2, 8)
            assert got == w
            want += w
            kept = table_of(e)
            e.recount()
            fresh = table_of(e)
            bad = np.nonzero(kept != fresh)[0]
            assert bad.size == 0, [(int(i), int(kept[i]), int(fresh[i])) for i in bad[:8]]
            if len(w) < 8:
                break
        assert seen == set(want_delta), ('corpus: merges not reached', set(want_delta) - seen)
        assert e.samples() == st.samples()
        return e.stats(), want
    finally:
        e.close()


def bursts_corpus(seed, alphabet):
    """Random text over `alphabet` symbols with a run bias, cut into short bursts scattered over a
    filler background (a third of them across a chunk boundary), in 4 samples: runs, chains and
    separators next to sites, every pair of the small alphabet below 1/16 of the chunks."""
    rng = np.random.default_rng(seed)
    samples = []
    for n in (250_000, 170_000, 110_001, 70_000):
        buf = filler(rng, n)
        # (about 100 occurrences per pair of the alphabet over the four samples: below 1/16 of
        # the 2344 chunks, and far above the cold pairs of the merged tokens for 16 merges)
        for k in range(8 * alphabet * alphabet * n // 600_001):
            L = int(rng.integers(2, 24))
            toks = []
            while len(toks) < L:
                t = int(rng.integers(0, alphabet))
                toks += [t] * (1 if rng.random() > 0.1 else int(rng.integers(2, 5)))
            toks = toks[:L]
            pos = int(rng.integers(0, n - 64))
            if k % 3 == 0:
                pos = min(n - 64, (pos // CHUNK + 1) * CHUNK - int(rng.integers(1, L)))
            buf[pos:pos + L] = toks
        # a burst first and last in the sample
        buf[:3] = [0, 1, 0]
        buf[-3:] = [1, 0, 1]
        samples.append(buf)
    return samples


@pytest.mark.parametrize('seed,alphabet', [(1, 4), (2, 6), (3, 8)])
def test_random_bursts_keep_the_table(seed, alphabet):
    samples = bursts_corpus(seed, alphabet)
    stats, merges = drive(samples, [1] * BASE, 0, 2, set())
    print(stats)
    nch = n_chunks_of(samples)
    light = sum(1 for a, b, W in merges if a != b and 16 * W < nch)
    # (the merged tokens are cold: once a pair of them may outweigh the hot pairs the loop hands
    # over to the host path, so the later light merges need not all be delta iterations)
    assert 4 <= stats['delta_passes'] <= light, (stats, light)
    assert stats['delta_chunks'] >= stats['delta_passes'], stats


def placed_runs_corpus():
    """Placed sites on the filler background, 2.8 M tokens (3 chunks per region), max_length 4:
    (7, 8)  chains a b a b .. of 2, 3 and 600 sites across chunks (W 625);
    (0, 1)  a in slot 255 and b in slot 0 of the next chunk, inside a region and across regions,
            every fourth with an a before it (W 520 with the 20 below);
    (6, 6)  an X X pair between them (full pass, W 420), then the chain's (c, c) (W 310);
    (2, 3)  a a .. a b with 600 and 601 a's (3 chunks) and with 0 .. 5 (W 270); len16[2] = 3 keeps
            (2, 2) itself out of the selection;
    (9, 9)  another X X pair (W 230);
    (4, 5)  a b b .. b with 600 and 601 b's and with 1 .. 6 (W 200); len16[5] = 3;
    (10, 11) first and last in its sample, alone in its sample, and behind a chunk the (0, 1)
            merge left partial (W 171)."""
    rng = np.random.default_rng(11)
    n = 2_800_000
    buf = filler(rng, n, HOT_BASE)

    def put(pos, toks):
        buf[pos:pos + len(toks)] = toks

    # (7, 8): 600 + 5 * 2 + 5 * 3 sites
    put(CHUNK * 40 - 5, [7, 8] * 600)
    for i in range(5):
        put(CHUNK * (60 + 2 * i) - 1 - i, [7, 8] * 2)
        put(CHUNK * (80 + 2 * i) - 2 - i, [7, 8] * 3)
    # (0, 1): 500 chunk boundaries (3 chunks per region: both kinds)
    for k in range(100, 600):
        put(CHUNK * k - 1, [0, 1])
        if k % 4 == 0:
            put(CHUNK * k - 2, [0])
    # (6, 6) and (9, 9)
    for i in range(420):
        put(CHUNK * 600 + 37 * i, [6, 6])
    for i in range(230):
        put(CHUNK * 700 + 41 * i, [9, 9])
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
    samples = [buf]
    # (10, 11) first and last in a sample, and alone in one
    for i in range(75):
        samples.append(np.concatenate([[10, 11], filler(rng, 17, HOT_BASE),
                                       [10, 11]]).astype(np.int32))
    samples.append(np.array([10, 11], np.int32))
    len16 = [1] * HOT_BASE
    len16[2] = len16[5] = 3
    return samples, len16


def test_placed_runs_chains_and_boundaries():
    samples, len16 = placed_runs_corpus()
    wanted = {(7, 8), (0, 1), (2, 3), (4, 5), (10, 11)}
    stats, merges = drive(samples, len16, 4, 2, wanted)
    print(stats)
    assert stats['delta_passes'] >= len(wanted), stats
    # the X X pairs between them take the full pass: delta, delta, full, full, delta, full,
    # delta, delta
    c78 = HOT_BASE
    assert [m[:2] for m in merges[:8]] == [(7, 8), (0, 1), (6, 6), (c78, c78), (2, 3), (9, 9),
                                           (4, 5), (10, 11)], merges[:8]


def placed_empties_corpus():
    """130 sections of two chunks of 12 13 12 13 .., each behind a chunk ending in 14 and before a
    chunk starting with 15: eight heavy merges (full passes) leave one token z in each chunk of
    a section; then (14, z), (z, z) and (z, 15) tie at W 130 (the tie pass).  (14, z) -> u goes
    first and empties the section's first chunk (its site lies across two chunks); (z, 15) -> v
    then has its left neighbour u beyond that emptied chunk, and (u, v) is a site whose two
    halves lie either side of it and which empties the section's second chunk too.  420 (0, 1)
    sites across chunk boundaries merge in the delta form between the heavy ones."""
    rng = np.random.default_rng(12)
    n = 1_800_000
    buf = filler(rng, n, HOT_BASE)
    for s in range(130):
        c0 = 50 + 40 * s
        buf[CHUNK * c0:CHUNK * (c0 + 2)] = [12, 13] * CHUNK
        buf[CHUNK * c0 - 1] = 14
        buf[CHUNK * (c0 + 2)] = 15
    for k in range(5500, 5920):
        buf[CHUNK * k - 1] = 0
        buf[CHUNK * k] = 1
    return [buf, filler(rng, 999, HOT_BASE)], [1] * HOT_BASE


def test_placed_sites_beyond_emptied_chunks():
    samples, len16 = placed_empties_corpus()
    stats, merges = drive(samples, len16, 0, 2, {(0, 1)})
    print(stats)
    assert stats['delta_passes'] >= 4, stats
    # both pairs around a section's token merged in turn, then the pair of their products
    tail = [m for m in merges if m[2] == 130]
    assert len(tail) == 3 and tail[0][0] == 14 and tail[1][1] == 15, merges
    assert tail[2][:2] == (HOT_BASE + merges.index(tail[0]), HOT_BASE + merges.index(tail[1]))


def test_knob_turns_the_delta_form_off(monkeypatch):
    monkeypatch.setenv('BPE_DELTA', '0')
    samples = bursts_corpus(1, 4)
    stats, merges = drive(samples, [1] * BASE, 0, 2, set())
    assert stats['delta_passes'] == 0 and stats['delta_chunks'] == 0, stats
    ids, off = flat(samples)
    st = OracleState(ids, off, [1] * BASE, BASE, extra=1024)
    assert merges == st.merge_until(0, 2, 16)
