"""Corpus out on the device (bpe_export_samples, bpe_export_text_batch, include/bpe.h;
csrc/bpe_export.hip.h): the trained corpus's samples as token ids, vector indices, code units or text.

Expected values never come from the code under test:
  - restate(): pick, map, concatenate, offsets over a list of samples (oracle.Corpus / OracleState
    sample lists), pinned on every golden case against the reference's final_ids and vectors;
  - the golden cases' final_ids, vectors and samples.
Equality with read_corpus / read_samples is a secondary check only.
"""
import ctypes
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from bpe_amd import ROOT, make_engine, pkg, run_engine
from golden_util import compact_index, load_small
from oracle import Corpus, OracleState

gpu = pytest.mark.gpu
T = pkg.EXPORT_TILE
KINDS = ['ids', 'vectors', 'code']
i32p, i64p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)


def sent(dtype):
    """The sentinel the tests pre-fill outputs with: every byte 0x5A."""
    return np.frombuffer(b'\x5a' * np.dtype(dtype).itemsize, dtype)[0]


@functools.lru_cache(maxsize=None)
def hip():
    from test_digest_stream import _hip
    return _hip()


class Dev:
    """A device buffer of the HIP runtime libbpe runs on, every byte the sentinel's; at(k): the
    address of byte k."""

    def __init__(self, nbytes):
        self.n = max(int(nbytes), 16)
        p = ctypes.c_void_p()
        assert hip().hipMalloc(ctypes.byref(p), self.n) == 0
        self.p = p.value
        assert self.p % 16 == 0
        host = np.full(self.n, 0x5A, np.uint8)
        assert hip().hipMemcpy(self.p, host.ctypes.data, self.n, 1) == 0   # hipMemcpyHostToDevice

    def at(self, k=0):
        return self.p + k

    def read(self, dtype, count=None, byte_off=0):
        size = np.dtype(dtype).itemsize
        out = np.zeros((self.n - byte_off) // size if count is None else count, dtype)
        if out.size:
            assert hip().hipMemcpy(out.ctypes.data, self.p + byte_off, out.nbytes, 2) == 0   # DeviceToHost
        return out

    def free(self):
        if self.p:
            hip().hipFree(self.p)
            self.p = 0


class Hole(Exception):
    def __init__(self, token, k, i):
        super().__init__('unknown token index: %d (sample %d, position %d)' % (token, k, i))


def restate(samples, idx=None, kind='ids', index=None):
    """The export of `samples` (lists of token ids): (values, offsets)."""
    pick = list(samples) if idx is None else [samples[i] for i in idx]
    off = np.zeros(len(pick) + 1, np.int64)
    np.cumsum([len(s) for s in pick], out=off[1:])
    flat = np.concatenate([np.asarray(s, np.int64) for s in pick] + [np.zeros(0, np.int64)])
    if kind == 'ids':
        return flat.astype(np.int32), off
    if kind == 'code':
        return (flat + 1).astype(np.uint16), off
    table = np.full(max(len(index), int(flat.max(initial=-1)) + 1), -1, np.int64)
    table[:len(index)] = index
    vals = table[flat]
    bad = np.flatnonzero(vals < 0)
    if bad.size:
        k = int(np.searchsorted(off, bad[0], 'right')) - 1
        raise Hole(int(flat[bad[0]]), k, int(bad[0] - off[k]))
    return vals.astype(np.int32), off


def case_index(case):
    to_vec = compact_index(case['token_table'])
    return [to_vec.get(i, -1) for i in range(len(case['token_table']))]


# ---- CPU ------------------------------------------------------------------------------------------

def test_new_names_are_exported_and_export_stats_match_the_header():
    for name in ('bpe_export_samples', 'bpe_export_samples_device', 'bpe_export_text_batch',
                 'bpe_export_text_batch_device', 'bpe_get_export_stats', 'bpe_reset_export_stats'):
        assert name in pkg.C_API
        assert hasattr(pkg.lib(), name), name
    for name in ('export_samples', 'export_samples_tensors', 'export_text', 'export_text_flat', 'export_text_tensors',
                 'export_stats', 'reset_export_stats'):
        assert hasattr(pkg.Engine, name), name
    src = open(os.path.join(ROOT, 'include', 'bpe.h')).read()
    body = re.search(r'typedef struct \{([^}]*)\} bpe_export_stats;', src).group(1)
    fields = re.findall(r'^\s*(int64_t|double)\s+(\w+);', body, re.M)
    assert [f[1] for f in fields] == [f[0] for f in pkg.ExportStats._fields_] == ['calls', 'samples', 'values', 'kernel_ms']
    assert [f[0] for f in fields] == ['int64_t', 'int64_t', 'int64_t', 'double']
    assert [f[1] for f in pkg.ExportStats._fields_] == [ctypes.c_int64] * 3 + [ctypes.c_double]
    assert ctypes.sizeof(pkg.ExportStats) == 8 * len(fields) == 32

    def define(name):
        return int(re.search(r'#define %s\s+(\d+)' % name, src).group(1))
    assert (pkg.EXPORT_IDS, pkg.EXPORT_VECTORS, pkg.EXPORT_CODE) == (0, 1, 2) == \
        (define('BPE_EXPORT_IDS'), define('BPE_EXPORT_VECTORS'), define('BPE_EXPORT_CODE'))
    assert pkg.EXPORT_TILE == 256 == define('BPE_EXPORT_TILE')
    assert pkg.EXPORT_SCAN_THREADS == 1024 == define('BPE_EXPORT_SCAN_THREADS')


def test_restatement_on_the_golden_cases():
    cases = load_small()
    assert len(cases) == 1509
    n_vec = 0
    for case in cases:
        final = case['final_ids']
        ids, off = restate(final)
        assert [ids[off[k]:off[k + 1]].tolist() for k in range(len(final))] == final, case['name']
        code, coff = restate(final, None, 'code')
        assert code.dtype == np.uint16 and np.array_equal(code, ids + 1) and np.array_equal(coff, off)
        if not case['token_table']:
            assert not ids.size and all(isinstance(v, str) for v in case['vectors'])
            continue
        vec, voff = restate(final, None, 'vectors', case_index(case))
        assert [vec[voff[k]:voff[k + 1]].tolist() for k in range(len(final))] == case['vectors'], case['name']
        rev = list(range(len(final)))[::-1]
        vec, voff = restate(final, rev + rev[:1], 'vectors', case_index(case))
        want = [case['vectors'][k] for k in rev + rev[:1]]
        assert [vec[voff[k]:voff[k + 1]].tolist() for k in range(len(want))] == want, case['name']
        n_vec += len(final)
    assert n_vec > 4300
    # a hole: the first failing value in output order
    with pytest.raises(Hole, match=r'unknown token index: 2 \(sample 1, position 0\)'):
        restate([[0, 1], [2, 0], [2]], None, 'vectors', [0, 1, -1])
    with pytest.raises(Hole, match=r'unknown token index: 5 \(sample 0, position 1\)'):
        restate([[0, 1], [2, 0], [1, 5]], [2, 1], 'vectors', [0, 1, -1])


# ---- GPU ------------------------------------------------------------------------------------------

def engine_of(samples, n_tokens=None):
    """A context holding `samples` (one device append: a packed corpus)."""
    e = pkg.Engine(0)
    if n_tokens:
        e.set_token_len16(n_tokens - 1, 1)
    e.add_samples([np.asarray(s, np.int32) for s in samples])
    return e


def full_index(samples, extra=0):
    """An index without holes at the ids of `samples`: id -> 3 * id + 1 (not the identity)."""
    top = max([max(s) for s in samples if len(s)] + [0]) + 1 + extra
    return (3 * np.arange(top) + 1).astype(np.int32)


def export_args(e, kind, idx, tvi, n=None):
    """(kind code, idx pointer, n, index pointer, its length, the arrays to keep alive)."""
    idx_a = None if idx is None else np.ascontiguousarray(idx, np.int64)
    n = (e.corpus_size()[0] if idx is None else idx_a.size) if n is None else n
    idx_p = None if idx is None else (idx_a if idx_a.size else np.zeros(1, np.int64)).ctypes.data_as(i64p)
    tvi_a = None if tvi is None else np.ascontiguousarray(tvi, np.int32)
    return (pkg.Engine._EXPORT_KINDS[kind], idx_p, n, None if tvi is None else tvi_a.ctypes.data_as(i32p),
            0 if tvi is None else tvi_a.size, (idx_a, tvi_a))


def raw_export(e, kind, idx, tvi, vals, cap, off, n=None):
    """bpe_export_samples on caller-made buffers: the return code."""
    k, idx_p, n, tvi_p, n_index, _keep = export_args(e, kind, idx, tvi, n)
    return pkg.lib().bpe_export_samples(e._ctx, k, idx_p, n, tvi_p, n_index,
                                        None if vals is None else vals.ctypes.data, cap, off.ctypes.data_as(i64p))


def raw_export_device(e, kind, idx, tvi, d_vals, cap, d_off, n=None):
    """bpe_export_samples_device on device addresses: (return code, needed; -7 when not written)."""
    k, idx_p, n, tvi_p, n_index, _keep = export_args(e, kind, idx, tvi, n)
    need = ctypes.c_int64(-7)
    rc = pkg.lib().bpe_export_samples_device(e._ctx, k, idx_p, n, tvi_p, n_index, d_vals, cap, d_off,
                                             ctypes.byref(need))
    return rc, need.value


def device_export(e, kind, idx, tvi, shift=0):
    """The device form into hipMalloc'ed buffers, the sizing call first: (values, offsets) read back.
    shift: elements the value pointer is moved off its 16-byte alignment; everything around the
    values must stay as it was."""
    dt = np.dtype(np.uint16 if kind == 'code' else np.int32)
    n_off = (e.corpus_size()[0] if idx is None else len(idx)) + 1
    d_off = Dev(8 * n_off)
    try:
        rc, need = raw_export_device(e, kind, idx, tvi, None, 0, d_off.at())
        assert rc == (pkg.ERR_ARG if need > 0 else pkg.BPE_OK), (rc, need, pkg.last_error())
        off = d_off.read(np.int64, n_off)
        assert off[-1] == need
        d_vals = Dev((shift + need + 4) * dt.itemsize)
        try:
            rc, need2 = raw_export_device(e, kind, idx, tvi, d_vals.at(shift * dt.itemsize), need, d_off.at())
            assert (rc, need2) == (pkg.BPE_OK, need), (rc, need2, pkg.last_error())
            assert np.array_equal(d_off.read(np.int64, n_off), off)
            host = d_vals.read(dt)
            assert (host[:shift] == sent(dt)).all() and (host[shift + need:] == sent(dt)).all(), (kind, shift)
            return host[shift:shift + need], off
        finally:
            d_vals.free()
    finally:
        d_off.free()


def check_routes(e, samples, idx=None, index=None, kinds=KINDS, what='', shifts=(0,)):
    """Host and device forms of every kind against the restatement."""
    for kind in kinds:
        tvi = index if kind == 'vectors' else None
        want, woff = restate(samples, idx, kind, index)
        got, off = e.export_samples(idx, kind, tvi)
        assert got.dtype == want.dtype and np.array_equal(off, woff), (what, kind)
        assert np.array_equal(got, want), (what, kind)
        for shift in shifts:
            d_got, d_off = device_export(e, kind, idx, tvi, shift)
            assert np.array_equal(d_off, woff), (what, kind, shift)
            assert np.array_equal(d_got, want), (what, kind, shift)


def lens_for_separators(pos):
    """Sample lengths that put the samples' separators at the slots `pos` of a packed corpus."""
    return [pos[0]] + [b - a - 1 for a, b in zip(pos, pos[1:])]


def edge_samples(rng, A=50):
    """Separators on slots 254, 255, 0 and 1 of chunks, a sample over four chunks, runs of empty
    samples across a chunk edge, an empty first and an empty last sample."""
    pos = [0, 254, 255, 256, 257, 1100, 5 * T - 1, 5 * T, 6 * T - 2, 7 * T - 1, 7 * T + 1, 8 * T + 254, 8 * T + 255,
           9 * T, 9 * T + 1, 9 * T + 2, 10 * T + 77, 10 * T + 78]
    lens = lens_for_separators(pos)
    assert lens[0] == 0 and lens[-1] == 0 and max(lens) >= 3 * T and lens.count(0) >= 6
    assert {p % T for p in pos} >= {254, 255, 0, 1}
    return [rng.integers(0, A, size=n).astype(np.int32).tolist() for n in lens]


@gpu
def test_chunk_edges_on_a_packed_corpus():
    rng = np.random.default_rng(1)
    samples = edge_samples(rng)
    e = engine_of(samples)
    try:
        index = full_index(samples)
        check_routes(e, samples, None, index, what='all')
        n = len(samples)
        check_routes(e, samples, list(range(n))[::-1], index, what='reversed')
        check_routes(e, samples, [5, 5, 0, n - 1, 5, 1], index, what='repeats')
        ids, off = e.read_corpus()                       # (secondary)
        got, goff = e.export_samples()
        assert np.array_equal(got, ids) and np.array_equal(goff, off)
        st = e.export_stats()
        assert st['calls'] > 0 and st['samples'] > 0 and st['values'] > 0 and st['kernel_ms'] > 0
        e.reset_export_stats()
        assert e.export_stats() == {'calls': 0, 'samples': 0, 'values': 0, 'kernel_ms': 0.0}
    finally:
        e.close()


@gpu
def test_empty_corpus_and_empty_samples_only():
    for samples in ([], [[]], [[]] * (T + 3), [[]] * (2 * T) + [[7]] + [[]] * 3):
        e = engine_of(samples)
        try:
            check_routes(e, samples, None, np.arange(8, dtype=np.int32), what=len(samples))
            check_routes(e, samples, [], np.arange(8, dtype=np.int32), what='[]')
            if samples:
                idx = [len(samples) - 1, 0, len(samples) // 2]
                check_routes(e, samples, idx, np.arange(8, dtype=np.int32), what='picked')
        finally:
            e.close()


def merged(samples, merges, n_tokens):
    """(engine, oracle) after apply_merge of each (a, b) on both; new ids from n_tokens on."""
    c = Corpus()
    for s in samples:
        c.add_ids(s)
    ids, off = c.flat()
    st = OracleState(ids, off, [1] * n_tokens, n_tokens, extra=1024)
    e = make_engine([np.asarray(s, np.int32) for s in samples], [1] * n_tokens)
    for a, b in merges:
        w = st.apply_merge(a, b)
        assert e.apply_merge(a, b, e.num_tokens()) == w
    return e, st


@gpu
def test_dead_slots_and_tail_tags():
    rng = np.random.default_rng(2)
    # half-dead chunks: the edge corpus over three ids, its most frequent pairs merged
    samples = edge_samples(rng, A=3)
    e, st = merged(samples, [(0, 1), (2, 2), (3, 0)], 3)
    try:
        now = st.samples()
        assert sum(len(s) for s in now) < 0.8 * sum(len(s) for s in samples)
        index = full_index(now)
        n = len(now)
        check_routes(e, now, None, index, what='all')
        check_routes(e, now, list(range(n))[::-1] + [5, 5], index, what='selected')
    finally:
        e.close()
    # 'ab' * 128 per chunk merged eight times: chunks 1, 2 and 3 each keep one live slot of 256
    samples = [[2] * (T - 1), [0, 1] * (3 * T // 2) + [3], [], [0, 1] * 40]
    e, st = merged(samples, [(0, 1)] + [(k, k) for k in range(4, 11)], 4)
    try:
        now = st.samples()
        assert now[1] == [11, 11, 11, 3]
        index = full_index(now)
        check_routes(e, now, None, index, what='all but one slot')
        check_routes(e, now, [3, 1, 1, 0, 2], index, what='all but one slot, selected')
    finally:
        e.close()


@gpu
def test_after_a_compaction():
    """1.2 M slots: the first batch's merges kill a third of them, the second batch compacts at its
    start (more than 1 % dead past 2^20 slots) and merges again; an append then packs the corpus."""
    rng = np.random.default_rng(3)
    body = np.tile(np.array([0, 1, 2], np.int32), 400_000)
    body[rng.integers(0, body.size, 5000)] = 3
    samples = [body[:700_001], np.zeros(0, np.int32), body[700_001:], np.array([3, 3], np.int32)]
    c = Corpus()
    for s in samples:
        c.add_ids(s)
    st = OracleState(*c.flat(), [1] * 4, 4, extra=64)
    e = make_engine(samples, [1] * 4)
    e.stats_enable(True)
    try:
        assert e.merge_until(0, 2, 2) == st.merge_until(0, 2, 2)
        assert e.stats()['compactions'] == 0
        now = st.samples()
        check_routes(e, now, None, full_index(now), kinds=['ids', 'code'], what='a third dead')
        check_routes(e, now, [3, 2, 1, 0, 2], full_index(now), kinds=['vectors'], what='a third dead, selected')
        assert e.merge_until(0, 2, 1) == st.merge_until(0, 2, 1)
        assert e.stats()['compactions'] == 1, e.stats()
        now = st.samples()
        check_routes(e, now, None, full_index(now), kinds=['vectors'], what='compacted, merged')
        check_routes(e, now, [3, 2, 1, 0, 2], full_index(now), kinds=['ids', 'code'], what='compacted, merged, selected')
        e.add_sample([3, 1])                 # (an append packs the corpus first)
        now = now + [[3, 1]]
        assert e.stats()['compactions'] == 2, e.stats()
        check_routes(e, now, None, full_index(now), what='packed')
        check_routes(e, now, [4, 2, 4, 0], full_index(now), kinds=['ids'], what='packed, selected')
    finally:
        e.close()


@gpu
@pytest.mark.parametrize('mode', ['host', 'loop', 'pix'])
def test_export_after_merge_until_equals_the_oracles_corpus(mode):
    rng = np.random.default_rng(4)
    samples = [rng.integers(0, 6, size=n).astype(np.int32) for n in (0, 300, 254, 0, 1, 2000, 513, 0)]
    c = Corpus()
    for s in samples:
        c.add_ids(s)
    st = OracleState(*c.flat(), [1] * 6, 6, extra=256)
    want = st.merge_until(0, 2, 25)
    e, merges = run_engine(samples, [1] * 6, {'min_weight': 2, 'max_iterations': 25}, mode=mode)
    try:
        assert merges == want
        now = st.samples()
        check_routes(e, now, None, full_index(now), what=mode)
        check_routes(e, now, [5, 1, 7, 0, 5], full_index(now), what=mode)
    finally:
        e.close()


def untouched_after(e, kind, idx, tvi, room, n=None):
    """Both forms on sentinel-filled outputs: (host rc, device rc, message) with every output checked
    to be as it was."""
    n_off = (len(idx) if idx is not None else e.corpus_size()[0]) + 1
    dt = np.uint16 if kind == 'code' else np.int32
    vals, off = np.full(room, sent(dt), dt), np.full(n_off, sent(np.int64), np.int64)
    rc = raw_export(e, kind, idx, tvi, vals, room, off, n)
    msg = pkg.last_error()
    assert (vals == sent(dt)).all() and (off == sent(np.int64)).all()
    d_vals, d_off = Dev(room * np.dtype(dt).itemsize), Dev(8 * n_off)
    try:
        rc_d, need = raw_export_device(e, kind, idx, tvi, d_vals.at(), room, d_off.at(), n)
        assert pkg.last_error() == msg
        assert need == -7 and (d_vals.read(np.uint8) == 0x5A).all() and (d_off.read(np.uint8) == 0x5A).all()
    finally:
        d_vals.free()
        d_off.free()
    return rc, rc_d, msg


@gpu
def test_selected_samples():
    rng = np.random.default_rng(5)
    # 5000 one-token samples, and a sample that is the whole corpus
    ones = [[int(v)] for v in rng.integers(0, 40, size=5000)]
    e = engine_of(ones)
    try:
        index = full_index(ones)
        check_routes(e, ones, None, index, what='5000 x 1')
        check_routes(e, ones, rng.permutation(5000).tolist(), index, what='5000 x 1, permuted')
        check_routes(e, ones, [4999, 0, 4999, 2500] * 3, index, what='5000 x 1, repeats')
        check_routes(e, ones, [], index, what='[]')
        ids, off = e.read_samples([7, 7, 4000])          # (secondary)
        got, goff = e.export_samples([7, 7, 4000])
        assert np.array_equal(got, ids) and np.array_equal(goff, off)
        for bad in ([-1], [5000], [3, 5000, 4], [0, -1]):
            for kind in KINDS:
                assert untouched_after(e, kind, bad, index if kind == 'vectors' else None, 16)[:2] == \
                    (pkg.ERR_ARG, pkg.ERR_ARG), (bad, kind)
        # every sample wants n = the sample count
        assert untouched_after(e, 'ids', None, None, 8000, n=4999)[:2] == (pkg.ERR_ARG, pkg.ERR_ARG)
        assert untouched_after(e, 'ids', None, None, 8000, n=0)[:2] == (pkg.ERR_ARG, pkg.ERR_ARG)
    finally:
        e.close()
    whole = [rng.integers(0, 9, size=5 * T + 17).astype(np.int32).tolist()]
    e = engine_of(whole)
    try:
        check_routes(e, whole, [0], full_index(whole), what='one sample')
        check_routes(e, whole, [0, 0], full_index(whole), what='one sample twice')
    finally:
        e.close()


@gpu
def test_sizes_past_the_tile_and_the_scan_constants():
    rng = np.random.default_rng(6)
    # one token past the tile; one region more than a scan thread owns (a region per chunk here)
    for n_tok, what in ((T - 1, 'tile - 1'), (T, 'tile'), (T + 1, 'tile + 1')):
        samples = [rng.integers(0, 9, size=n_tok).astype(np.int32).tolist(), [1, 2]]
        e = engine_of(samples)
        try:
            check_routes(e, samples, None, full_index(samples), what=what)
            check_routes(e, samples, [1, 0], full_index(samples), what=what)
        finally:
            e.close()
    S = pkg.EXPORT_SCAN_THREADS
    lens = [0, T * (S + 5) // 2, 3, 0, T * (S + 5) // 2, 9]             # S + 5 chunks and a bit
    samples = [rng.integers(0, 30, size=n).astype(np.int32) for n in lens]
    e = engine_of(samples)
    try:
        lists = [s.tolist() for s in samples]
        check_routes(e, lists, None, full_index(lists), what='regions past the scan threads')
        check_routes(e, lists, [4, 2, 1, 5, 0], full_index(lists), kinds=['ids', 'code'], what='... selected')
    finally:
        e.close()
    # more selected samples than scan threads: S + 1 and S + 2 entries to scan
    few = [[int(v)] * int(m) for v, m in zip(rng.integers(0, 9, size=40), rng.integers(0, 4, size=40))]
    e = engine_of(few)
    try:
        for n in (S - 1, S, S + 1, 2 * S + 3):
            check_routes(e, few, rng.integers(0, 40, size=n).tolist(), full_index(few), kinds=['ids'], what=n)
    finally:
        e.close()


@gpu
def test_vectors_holes_and_the_missing_index():
    samples = [[0, 1, 2], [3, 3], [], [1, 0, 1, 0], [4, 6], [0] * 300, [2, 2], [0, 5, 1], [6]]
    e = engine_of(samples, n_tokens=12)
    try:
        # holes at absent ids only (7 .. 11, and every id past the index)
        index = np.array([5, 4, 3, 2, 1, 0, 6, -1, -1, -1], np.int32)
        check_routes(e, samples, None, index, kinds=['vectors'], what='absent holes')
        check_routes(e, samples, [8, 0, 0, 5], index, kinds=['vectors'], what='absent holes, selected')
        # id 5 is a hole: the last token of ... sample 7's middle; make it the last of sample 3
        samples2 = [[0, 1, 2], [3, 3], [], [1, 0, 1, 5], [4, 6], [0] * 300, [2, 2], [0, 5, 1], [6]]
        e2 = engine_of(samples2, n_tokens=12)
        try:
            holed = index.copy()
            holed[5] = -1
            want = r'unknown token index: 5 \(sample 3, position 3\)'
            with pytest.raises(Hole, match=want):
                restate(samples2, None, 'vectors', holed)
            rc, rc_d, msg = untouched_after(e2, 'vectors', None, holed, 400)
            assert (rc, rc_d) == (pkg.ERR_VOCAB, pkg.ERR_VOCAB) and re.fullmatch(want, msg), msg
            assert pkg.last_error() == msg                      # (the device form's message too)
            # selected: K is the place in idx; the first failing value in output order
            idx = [8, 7, 3, 7]
            with pytest.raises(Hole, match=r'unknown token index: 5 \(sample 1, position 1\)'):
                restate(samples2, idx, 'vectors', holed)
            rc, rc_d, msg = untouched_after(e2, 'vectors', idx, holed, 400)
            assert (rc, rc_d) == (pkg.ERR_VOCAB, pkg.ERR_VOCAB)
            assert msg == 'unknown token index: 5 (sample 1, position 1)', msg
            # an index too short for a present id: ids at or past n_index are holes
            rc, rc_d, msg = untouched_after(e2, 'vectors', None, holed[:5], 400)
            assert (rc, rc_d) == (pkg.ERR_VOCAB, pkg.ERR_VOCAB)
            assert msg == 'unknown token index: 5 (sample 3, position 3)', msg
            # a list that skips every sample with the hole succeeds, and the context stays usable
            check_routes(e2, samples2, [0, 1, 2, 4, 5, 6, 8, 8], holed, kinds=['vectors'], what='skips the hole')
            check_routes(e2, samples2, None, index, what='after the failures')
        finally:
            e2.close()
        # no index
        for idx in (None, [1, 0]):
            assert untouched_after(e, 'vectors', idx, None, 400)[:2] == (pkg.ERR_STATE, pkg.ERR_STATE)
    finally:
        e.close()


@gpu
def test_codes_up_to_the_vocabulary_limit_and_odd_alignment():
    rng = np.random.default_rng(7)
    top = pkg.MAX_VOCAB - 1
    samples = [[top, 0, top - 1], [], rng.integers(0, top + 1, size=2 * T + 5).tolist(), [30000, top], [top]]
    e = pkg.Engine(0)
    try:
        e.set_token_len16(top, 1)
        assert e.num_tokens() == pkg.MAX_VOCAB
        e.add_samples([np.asarray(s, np.int32) for s in samples])
        # destinations moved by one to three elements: every residue of the stores' 4- and 16-byte
        # grids, odd 2-byte alignment for the codes and odd 4-byte alignment for the ids among them
        check_routes(e, samples, None, None, kinds=['ids', 'code'], what='all', shifts=(0, 1, 2, 3))
        check_routes(e, samples, [4, 2, 0, 3, 2], None, kinds=['ids', 'code'], what='selected', shifts=(0, 1, 2, 3))
        code, off = e.export_samples(None, 'code')
        assert code.dtype == np.uint16 and int(code.max()) == pkg.MAX_VOCAB == 0xD800
        assert np.array_equal(code.astype(np.int64), restate(samples)[0].astype(np.int64) + 1)
        # a misaligned pointer is refused: 2-byte values on an odd address, 4-byte values 2 bytes off
        d_vals, d_off = Dev(4096), Dev(64)
        try:
            assert raw_export_device(e, 'code', None, None, d_vals.at(1), 2000, d_off.at())[0] == pkg.ERR_ARG
            assert raw_export_device(e, 'ids', None, None, d_vals.at(2), 1000, d_off.at())[0] == pkg.ERR_ARG
            assert (d_vals.read(np.uint8) == 0x5A).all() and (d_off.read(np.uint8) == 0x5A).all()
        finally:
            d_vals.free()
            d_off.free()
    finally:
        e.close()


@gpu
def test_capacity_and_the_sizing_call():
    rng = np.random.default_rng(8)
    samples = [rng.integers(0, 9, size=n).astype(np.int32).tolist() for n in (3, 0, T + 9, 40)]
    e = engine_of(samples)
    try:
        index = full_index(samples)
        for idx in (None, [3, 0, 2, 2]):
            for kind in KINDS:
                tvi = index if kind == 'vectors' else None
                want, woff = restate(samples, idx, kind, index)
                need = want.size
                dt = want.dtype
                for cap, vals in ((need - 1, np.full(need, sent(dt), dt)), (0, None)):
                    off = np.full(len(woff), sent(np.int64), np.int64)
                    assert raw_export(e, kind, idx, tvi, vals, cap, off) == pkg.ERR_ARG, (kind, cap)
                    assert np.array_equal(off, woff) and (vals is None or (vals == sent(dt)).all()), (kind, cap)
                    d_vals, d_off = Dev(need * dt.itemsize), Dev(8 * len(woff))
                    try:
                        rc, needed = raw_export_device(e, kind, idx, tvi, None if vals is None else d_vals.at(), cap,
                                                       d_off.at())
                        assert (rc, needed) == (pkg.ERR_ARG, need), (kind, cap)
                        assert np.array_equal(d_off.read(np.int64, len(woff)), woff)
                        assert (d_vals.read(np.uint8) == 0x5A).all()
                    finally:
                        d_vals.free()
                        d_off.free()
                # exactly enough room
                vals, off = np.full(need + 2, sent(dt), dt), np.full(len(woff), sent(np.int64), np.int64)
                assert raw_export(e, kind, idx, tvi, vals, need, off) == pkg.BPE_OK
                assert np.array_equal(vals[:need], want) and (vals[need:] == sent(dt)).all()
                assert np.array_equal(off, woff)
    finally:
        e.close()


def stats_but_export(e):
    return e.stats(), e.ingest_stats(), e.append_stats(), e.corpus_size(), e.num_tokens(), e.token_counts().tolist()


def export_everything(e, index):
    e.export_samples(None, 'ids')
    device_export(e, 'code', None, None)
    e.export_samples([0, 0], 'vectors', index)
    device_export(e, 'ids', [1, 0], None)


@gpu
def test_read_only_in_the_stream_mode_with_the_digest_lists():
    from test_digest_stream import light_pairs_corpus
    samples, len16 = light_pairs_corpus(40)
    c = Corpus()
    for s in samples:
        c.add_ids(s)
    st = OracleState(*c.flat(), len16, len(len16), extra=256)
    want = st.merge_until(0, 2, 40)
    assert len(want) == 40
    index = np.arange(len(len16) + 64, dtype=np.int32)
    one = make_engine(samples, len16)
    one.stats_enable(True)
    e = make_engine(samples, len16)
    e.stats_enable(True)
    try:
        assert one.merge_until(0, 2, 40) == want
        assert e.merge_until(0, 2, 20) == want[:20]
        before = stats_but_export(e)
        assert before[0]['digest_scans'] > 0 and before[0]['digest_scans'] < before[0]['digest_passes'], before[0]
        export_everything(e, index)
        assert stats_but_export(e) == before
        assert e.merge_until(0, 2, 20) == want[20:]
        a, b = one.stats(), e.stats()
        # the lists survived the export: the split run builds the plane once, as the single run does
        assert b['digest_builds'] == a['digest_builds'] == 1, (a, b)
        assert b['digest_passes'] == a['digest_passes'] == 40, (a, b)
        now = st.samples()
        check_routes(e, now, None, index, kinds=['ids'], what='final')
        got, off = one.export_samples()
        assert np.array_equal(got, st.ids[:st.off[-1]]) and np.array_equal(off, st.off)
    finally:
        one.close()
        e.close()


@gpu
def test_read_only_in_the_incremental_mode_and_the_maintained_state():
    from test_maintained_state import check_maintained, random_cold_corpus
    from test_digest_stream import flat
    samples, len16, _merges, _rng = random_cold_corpus(1)
    ids, off = flat(samples)
    index = np.arange(len(len16) + 64, dtype=np.int32)
    for mode in ('incremental', 'stream'):
        st = OracleState(ids, off, len16, len(len16), extra=1024)
        want = st.merge_until(0, 2, 20)
        e = make_engine(samples, len16)
        e.stats_enable(True)
        try:
            e.set_mode(mode)
            assert e.merge_until(0, 2, 20) == want
            if mode == 'stream':
                check_maintained(e, st)                # (in the maintained state, tables == a recount)
            before = stats_but_export(e)
            export_everything(e, index)
            assert stats_but_export(e) == before
            if mode == 'stream':
                check_maintained(e, st)
            check_routes(e, st.samples(), None, index, kinds=['ids', 'vectors'], what=mode)
            more = st.merge_until(0, 2, 20)
            assert len(more) == 20 and e.merge_until(0, 2, 20) == more
            if mode == 'stream':
                check_maintained(e, st)
            else:
                assert e.stats()['pix_merges'] == 40, e.stats()
            check_routes(e, st.samples(), None, index, kinds=['code'], what=mode)
        finally:
            e.close()


def case_decoder(case, dec):
    tt = case['token_table']
    n_chars = len(tt) - len(case['merges'])
    dec.clear()
    if n_chars:
        dec.add_tokens([t[0] for t in tt[:n_chars]])
    if case['merges']:
        dec.add_merges([(a, b, n_chars + i) for i, (a, b, _w) in enumerate(case['merges'])])
    return n_chars


@gpu
def test_golden_cases():
    """Every tenth case: text in (add_text), the case's merge_until, then ids == final_ids, vectors
    == the reference's vectors, text through a Decoder of the case's table == the samples."""
    cases = load_small()[::10]
    assert len(cases) >= 150
    dec = pkg.Decoder(0)
    bad = []
    n_vec = 0
    try:
        for case in cases:
            e = pkg.Engine(0)
            try:
                e.add_text(case['samples'])
                o = case['opts']
                merges = e.merge_until(o.get('max_length') or 0, o.get('min_weight') or 0, o.get('max_iterations') or 0)
                ok = [list(m) for m in merges] == case['merges']
                n = len(case['samples'])
                ids, off = e.export_samples()
                ok = ok and [ids[off[k]:off[k + 1]].tolist() for k in range(n)] == case['final_ids']
                case_decoder(case, dec)
                ok = ok and e.export_text(dec) == case['samples']
                rev = list(range(n))[::-1]
                ok = ok and e.export_text(dec, rev) == case['samples'][::-1]
                if case['token_table']:
                    vec, voff = e.export_samples(None, 'vectors', case_index(case))
                    ok = ok and [vec[voff[k]:voff[k + 1]].tolist() for k in range(n)] == case['vectors']
                    vec, voff = e.export_samples(rev, 'vectors', case_index(case))
                    ok = ok and [vec[voff[k]:voff[k + 1]].tolist() for k in range(n)] == case['vectors'][::-1]
                    n_vec += n
            finally:
                e.close()
            if not ok:
                bad.append(case['name'])
    finally:
        dec.close()
    assert not bad, bad
    assert n_vec > 400


def raw_text_device(e, dec, idx, d_units, cap, d_off):
    """bpe_export_text_batch_device on device addresses: (return code, needed; -7 when not written)."""
    _k, idx_p, n, _t, _n, _keep = export_args(e, 'ids', idx, None)
    need = ctypes.c_int64(-7)
    rc = pkg.lib().bpe_export_text_batch_device(e._ctx, dec._dec if dec is not None else None, idx_p, n, d_units, cap,
                                                d_off, ctypes.byref(need))
    return rc, need.value


def device_text(e, dec, idx):
    """The device form of the text export into hipMalloc'ed buffers: the texts as a list of str."""
    n = e.corpus_size()[0] if idx is None else len(idx)
    d_off = Dev(8 * (n + 1))
    try:
        rc, need = raw_text_device(e, dec, idx, None, 0, d_off.at())
        if rc != (pkg.ERR_ARG if need > 0 else pkg.BPE_OK):
            raise pkg.BpeError(pkg.last_error(), rc)
        d_units = Dev(2 * (need + 3))
        try:
            rc, need2 = raw_text_device(e, dec, idx, d_units.at(), need, d_off.at())
            assert (rc, need2) == (pkg.BPE_OK, need), (rc, need2, pkg.last_error())
            o = d_off.read(np.int64, n + 1)
            host = d_units.read(np.uint16)
            assert o[0] == 0 and o[-1] == need and (host[need:] == sent(np.uint16)).all()
            return [pkg.units_to_str(host[o[k]:o[k + 1]]) for k in range(n)]
        finally:
            d_units.free()
    finally:
        d_off.free()


@gpu
def test_text_round_trip_and_the_decoders_errors():
    texts = ['a\U0001F600b\U0001F600b', '', '\ud800x\udc00', 'ab' * 300 + '\udfff', 'b\U00010000', '']
    e = pkg.Engine(0)
    dec = pkg.Decoder(0)
    short = pkg.Decoder(0)
    try:
        new_chars, _hist = e.add_text(texts)
        chars = [chr(int(cp)) for cp in new_chars]
        merges = e.merge_until(0, 2, 6)
        assert len(merges) >= 3
        abc = [(a, b, len(chars) + k) for k, (a, b, _w) in enumerate(merges)]
        dec.add_tokens(chars)
        dec.add_merges(abc)
        for idx in (None, [3, 0, 0, 5, 2], [], [4, 4]):
            want = texts if idx is None else [texts[k] for k in idx]
            assert e.export_text(dec, idx) == want, idx
            assert device_text(e, dec, idx) == want, idx
        # capacity: the decoder's sizing behaviour (offsets written, no unit)
        total = sum(len(t.encode('utf-16-le', 'surrogatepass')) // 2 for t in texts)
        buf = np.full(total, sent(np.uint16), np.uint16)
        ooff = np.full(len(texts) + 1, sent(np.int64), np.int64)
        rc = pkg.lib().bpe_export_text_batch(e._ctx, dec._dec, None, len(texts), buf.ctypes.data, total - 1,
                                             ooff.ctypes.data_as(i64p))
        assert rc == pkg.ERR_ARG and (buf == sent(np.uint16)).all() and ooff[-1] == total and ooff[0] == 0
        assert np.array_equal(np.diff(ooff), [len(t.encode('utf-16-le', 'surrogatepass')) // 2 for t in texts])
        # a decoder that knows fewer tokens: its own message, for the first unknown id in flat order
        short.add_tokens(chars[:2])
        ids, ioff = restate(e.samples())
        p = int(np.flatnonzero(ids >= 2)[0])
        k = int(np.searchsorted(ioff, p, 'right')) - 1
        want = 'unknown token index: %d (text %d, position %d)' % (ids[p], k, p - ioff[k])
        for call in (e.export_text, lambda d: device_text(e, d, None)):
            with pytest.raises(pkg.BpeError) as err:
                call(short)
            assert err.value.code == pkg.ERR_VOCAB and str(err.value).endswith(want), err.value
        # no decoder, a decoder elsewhere
        for call in (e.export_text, lambda d: device_text(e, d, None)):
            with pytest.raises(pkg.BpeError) as err:
                call(None)
            assert err.value.code == pkg.ERR_ARG
        if pkg.device_count() > 1:
            far = pkg.Decoder(1)
            try:
                far.add_tokens(chars)
                far.add_merges(abc)
                with pytest.raises(pkg.BpeError) as err:
                    e.export_text(far)
                assert err.value.code == pkg.ERR_ARG
            finally:
                far.close()
        assert e.export_text(dec) == texts
    finally:
        short.close()
        dec.close()
        e.close()


@gpu
def test_two_shards_on_one_device():
    rng = np.random.default_rng(9)
    samples = edge_samples(rng, A=5)
    one = make_engine([np.asarray(s, np.int32) for s in samples], [1] * 5)
    two = pkg.Engine(devices=[0, 0], reduce='host')
    dec = pkg.Decoder(0)
    try:
        for i in range(5):
            two.set_token_len16(i, 1)
        for s in samples:
            two.add_sample(np.asarray(s, np.int32))
        c = Corpus()
        for s in samples:
            c.add_ids(s)
        st = OracleState(*c.flat(), [1] * 5, 5, extra=64)
        want = st.merge_until(0, 2, 6)
        assert one.merge_until(0, 2, 6) == want and two.merge_until(0, 2, 6) == want
        assert two.shard_count() == 2
        now = st.samples()
        index = full_index(now)
        n = len(now)
        for idx in (None, list(range(n))[::-1], [n - 1, 0, 5, 5, n - 2], []):
            for kind in KINDS:
                tvi = index if kind == 'vectors' else None
                w, woff = restate(now, idx, kind, index)
                for e in (one, two):
                    got, off = e.export_samples(idx, kind, tvi)
                    assert np.array_equal(got, w) and np.array_equal(off, woff), (idx, kind)
        # a hole in the second shard's samples: K counts in the caller's list
        holed = index.copy()
        last = now[n - 2][-1]
        holed[last] = -1
        for idx in (None, list(range(n))[::-1]):
            with pytest.raises(Hole) as h:
                restate(now, idx, 'vectors', holed)
            for e in (one, two):
                with pytest.raises(pkg.BpeError) as err:
                    e.export_samples(idx, 'vectors', holed)
                assert err.value.code == pkg.ERR_VOCAB and str(err.value).endswith(str(h.value)), (err.value, h.value)
        dec.add_tokens(list('abcde'))
        dec.add_merges([(a, b, 5 + k) for k, (a, b, _w) in enumerate(want)])
        texts = [''.join('abcde'[i] for i in s) for s in samples]
        for idx in (None, [5, 0, 5, n - 2]):
            w = texts if idx is None else [texts[k] for k in idx]
            assert one.export_text(dec, idx) == w and two.export_text(dec, idx) == w
        # the device forms refuse a multi-device context, whatever the buffers
        d_vals, d_off = Dev(64), Dev(8 * (n + 1))
        try:
            assert raw_export_device(two, 'ids', None, None, d_vals.at(), 16, d_off.at()) == (pkg.ERR_ARG, -7)
            assert raw_text_device(two, dec, None, d_vals.at(), 32, d_off.at()) == (pkg.ERR_ARG, -7)
            assert (d_vals.read(np.uint8) == 0x5A).all() and (d_off.read(np.uint8) == 0x5A).all()
        finally:
            d_vals.free()
            d_off.free()
        assert two.export_stats()['calls'] > 0 and two.export_stats()['values'] > 0
    finally:
        dec.close()
        one.close()
        two.close()


def tensor_forms_check():
    """export_samples_tensors and export_text_tensors: torch tensors on the context's device."""
    import torch
    assert torch.cuda.is_available(), 'torch sees no device'
    texts = ['a\U0001F600b' * 90, '', 'ab' * 300 + '\udfff', 'b\U00010000']
    e = pkg.Engine(0)
    dec = pkg.Decoder(0)
    new_chars, _hist = e.add_text(texts)
    chars = [chr(int(cp)) for cp in new_chars]
    merges = e.merge_until(0, 2, 5)
    dec.add_tokens(chars)
    dec.add_merges([(a, b, len(chars) + k) for k, (a, b, _w) in enumerate(merges)])
    c = Corpus()
    for t in texts:
        c.add(t)
    st = OracleState.from_corpus(c)
    assert st.merge_until(0, 2, 5) == merges
    now = st.samples()
    index = full_index(now)
    for idx in (None, [2, 0, 2], []):
        for kind in KINDS:
            want, woff = restate(now, idx, kind, index)
            vals, off = e.export_samples_tensors(idx, kind, index if kind == 'vectors' else None)
            assert vals.is_cuda and off.is_cuda and off.dtype == torch.int64
            assert vals.dtype == (torch.int16 if kind == 'code' else torch.int32)
            assert np.array_equal(off.cpu().numpy(), woff)
            assert np.array_equal(vals.cpu().numpy().view(want.dtype), want)
            # into the caller's tensor, one element off its alignment
            buf = torch.full((want.size + 3,), 0x5A5A, dtype=vals.dtype, device='cuda')
            got, off = e.export_samples_tensors(idx, kind, index if kind == 'vectors' else None,
                                                out=buf[1:1 + want.size])
            assert got.numel() == want.size
            assert not want.size or got.data_ptr() == buf.data_ptr() + buf.element_size()
            host = buf.cpu().numpy()
            assert np.array_equal(host[1:1 + want.size].view(want.dtype), want)
            assert host[0] == 0x5A5A and (host[1 + want.size:] == 0x5A5A).all()
        w = texts if idx is None else [texts[k] for k in idx]
        units, off = e.export_text_tensors(dec, idx)
        assert units.is_cuda and units.dtype == torch.int16 and off.dtype == torch.int64
        host, o = units.cpu().numpy().view(np.uint16), off.cpu().numpy()
        assert [pkg.units_to_str(host[o[k]:o[k + 1]]) for k in range(len(w))] == w
    # ids -> text without leaving the device, through the decoder's own device form
    vals, off = e.export_samples_tensors()
    units, uoff = dec.decode_tensors(vals, off, 'ids')
    assert pkg.units_to_str(units.cpu().numpy().view(np.uint16)) == ''.join(texts)
    for x in (e, dec):
        x.close()
    return True


@gpu
def test_tensor_forms():
    """In a process of its own that imports torch before libbpe loads (PyTorch sees a device only
    when its HIP runtime is the process's first)."""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join(
        [here, os.path.join(os.path.dirname(here), 'oracle'), os.environ.get('PYTHONPATH', '')]))
    out = subprocess.run([sys.executable, os.path.abspath(__file__), 'tensor-forms'], env=env,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith('tensor forms ok'), \
        out.stdout[-2000:] + out.stderr[-3000:]


if __name__ == '__main__' and sys.argv[1:] == ['tensor-forms']:
    import torch  # noqa: F401  (before libbpe loads)
    print('tensor forms ok' if tensor_forms_check() else 'failed')
