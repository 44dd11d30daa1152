"""Skip-gram pair counts on the device (include/bpe.h "skip-gram pair counts",
csrc/bpe_skipgram_counts.hip.h) against a restatement of the rule: for every text, every place i and
every distance d in 1 .. w with i + d inside the text, the pairs (v[i], v[i + d]) and (v[i + d], v[i]),
counted by numpy.  Shapes sit around the count kernel's tile edge, its LDS table and the ends of
[0, dim); every route (host, device, tensors, text, UTF-8, corpus) gives the same bytes."""
import collections
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from bpe_amd import ROOT, pkg
from test_skipgram import CORPUS, full_index, trained_case, trained_encoder, trained_engine

TILE = getattr(pkg, 'SKIPGRAM_COUNTS_TILE', 2048)
SLOTS = getattr(pkg, 'SKIPGRAM_COUNTS_SLOTS', 4096)
MAX_DIM = getattr(pkg, 'SKIPGRAM_COUNTS_MAX_DIM', 16384)
WMAX = pkg.SKIPGRAM_MAX_WINDOW
WINDOWS = (1, 2, 5, WMAX)
LANES = 256          # lanes of a workgroup of the count kernel
CANARY = -0x5A5A5A5B
PAD = 8              # canary elements on each side of a plane
i64p = ctypes.POINTER(ctypes.c_int64)
pytestmark = pytest.mark.gpu


def want_counts(texts, w, dim):
    """The rule, counted: (targets, contexts, counts) in ascending (target, context) order."""
    dense = np.zeros(dim * dim, np.int64) if dim * dim <= 1 << 16 else None
    keys = [np.zeros(0, np.int64)]
    for v in texts:
        v = np.asarray(v, np.int64)
        for d in range(1, min(w, len(v) - 1) + 1):
            k = np.concatenate([v[:-d] * dim + v[d:], v[d:] * dim + v[:-d]])
            if dense is None:
                keys.append(k)
            else:
                dense += np.bincount(k, minlength=dim * dim)
    if dense is None:
        k, n = np.unique(np.concatenate(keys), return_counts=True)
    else:
        k = np.flatnonzero(dense)
        n = dense[k]
    return (k // dim).astype(np.int32), (k % dim).astype(np.int32), n.astype(np.int64)


def pairs_of(n, w):
    """The closed form of include/bpe.h: the pairs of a text of n values."""
    return 0 if n <= 1 else n * (n - 1) if n <= w + 1 else w * (2 * n - w - 1)


def flat(texts, lead=()):
    vals = np.array(list(lead) + [x for v in texts for x in v], np.int32)
    off = np.cumsum([len(lead)] + [len(v) for v in texts]).astype(np.int64)
    return vals, off


def text(n, dim, salt=0):
    i = np.arange(n)
    return ((i * 7 + i // 5 + salt * 13) % dim).tolist()


def check(got, texts, w, dim):
    """got equals the restatement; sum counts == P, ascending keys with none twice, symmetry."""
    t, c, n = (np.asarray(x.cpu() if hasattr(x, 'cpu') else x) for x in got)
    wt, wc, wn = want_counts(texts, w, dim)
    assert t.dtype == np.int32 and c.dtype == np.int32 and n.dtype == np.int64
    assert np.array_equal(t, wt) and np.array_equal(c, wc) and np.array_equal(n, wn)
    assert int(n.sum()) == sum(pairs_of(len(v), w) for v in texts)
    key, yek = t.astype(np.int64) * dim + c, c.astype(np.int64) * dim + t
    assert (np.diff(key) > 0).all()
    order = np.argsort(yek)
    assert np.array_equal(yek[order], key) and np.array_equal(n[order], n)
    return t, c, n


def edge_batch(w, dim=23):
    """Texts of TILE - w - 1 .. TILE + w + 1 values, each one placed to end exactly on a tile edge, to
    start exactly on one (behind a text that ends there) and to straddle one with the edge inside a
    window; fillers bring the next text to its place."""
    texts, pos = [], 0
    for n in range(TILE - w - 1, TILE + w + 2):
        for start in (-n, 0, TILE - w // 2 - 1):
            gap = (start - pos) % TILE
            if gap:
                texts.append(text(gap, dim, len(texts)))
            texts.append(text(n, dim, len(texts)))
            pos += gap + n
    return texts, w, dim


def empties_batch(w, dim=7):
    """Runs of more empty texts than a workgroup has lanes on the edge and just before it, and texts of
    0, 1 and 2 values."""
    run = [[]] * (LANES + 44)
    small = [[], [1], [2, 3], [], [4], [5, 6], [0]]
    return [text(TILE, dim)] + run + [text(TILE - 3, dim, 1)] + run + small * 3 + [text(40, dim, 2)] + run, w, dim


def equal_batch(w, dim=5):
    """One text of 3 TILE equal values, the value dim - 1: one cell holds all P pairs."""
    return [[dim - 1] * (3 * TILE)], w, dim


SHAPES = {'edge': edge_batch, 'empties': empties_batch, 'equal': equal_batch}
# a tile with more distinct forward pairs than the LDS table has slots; dim 1; the top of MAX_DIM
OVERFLOW_DIM = 89
FIXED = {
    'overflow': ([(np.arange(2 * TILE + 9) % OVERFLOW_DIM).tolist()], WMAX, OVERFLOW_DIM),
    'dim1': ([[0] * 5, [], [0], [0, 0], [0] * (TILE + 3)], 3, 1),
    'max_dim': ([[MAX_DIM - 1, 0, MAX_DIM - 2, MAX_DIM - 1, MAX_DIM - 1], [MAX_DIM - 1, MAX_DIM - 1], [3]], 2, MAX_DIM),
}


@pytest.fixture(scope='module')
def enc():
    e = pkg.Encoder(0)
    yield e
    e.close()


def host_twice(enc, texts, w, dim):
    vals, off = flat(texts, lead=[-5, dim])
    a, b = enc.skipgram_counts(vals, off, w, dim), enc.skipgram_counts(vals, off, w, dim)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    return check(a, texts, w, dim)


@pytest.mark.parametrize('w', WINDOWS)
@pytest.mark.parametrize('shape', sorted(SHAPES))
def test_shapes_at_the_tile_edge(enc, shape, w):
    texts, w, dim = SHAPES[shape](w)
    enc.reset_skipgram_counts_stats()
    t, c, n = host_twice(enc, texts, w, dim)
    st = enc.skipgram_counts_stats()
    assert st['calls'] == 4 and st['pairs_counted'] == 2 * int(n.sum()) and st['distinct_out'] == 2 * len(n)
    if shape == 'equal':
        assert (t.tolist(), c.tolist(), n.tolist()) == ([dim - 1], [dim - 1], [pairs_of(3 * TILE, w)])


@pytest.mark.parametrize('name', sorted(FIXED))
def test_the_table_overflows_and_the_ends_of_dim(enc, name):
    texts, w, dim = FIXED[name]
    enc.reset_skipgram_counts_stats()
    t, c, n = host_twice(enc, texts, w, dim)
    if name == 'overflow':
        assert dim * dim > SLOTS and len(n) > SLOTS and enc.skipgram_counts_stats()['lds_overflow'] > 0
    if name == 'max_dim':
        assert t[-1] == c[-1] == MAX_DIM - 1 and n[-1] == 4   # (the last cell of the accumulator)


def raw(enc, vals, off, w, dim, cap):
    t, c = np.full(cap + 2 * PAD, CANARY, np.int32), np.full(cap + 2 * PAD, CANARY, np.int32)
    n = np.full(cap + 2 * PAD, CANARY, np.int64)
    need = ctypes.c_int64(-1)
    rc = pkg.lib().bpe_encoder_skipgram_counts(enc._enc, vals.ctypes.data, off.ctypes.data_as(i64p), len(off) - 1, w, dim,
                                               t[PAD:].ctypes.data, c[PAD:].ctypes.data, n[PAD:].ctypes.data, cap,
                                               ctypes.byref(need))
    return rc, need.value, (t, c, n)


def test_values_outside_dim_capacity_and_arguments(enc):
    dim, w = 11, 2
    texts = [text(5, dim), [], text(TILE + 7, dim, 1), text(9, dim, 2), text(3 * TILE, dim, 3)]
    U = len(want_counts(texts, w, dim)[0])
    for bad in (dim, -1):
        spoiled = [list(v) for v in texts]
        spoiled[3][4] = spoiled[4][TILE + 1] = spoiled[4][5] = bad   # (the smallest place is named)
        vals, off = flat(spoiled)
        rc, need, planes = raw(enc, vals, off, w, dim, U)
        assert rc == pkg.ERR_ARG and all((p == CANARY).all() for p in planes)
        assert pkg.last_error() == 'bpe native: skip-gram counts value %d outside [0, %d) (text 3, position 4)' % (bad, dim)
    vals, off = flat(texts)
    rc, need, planes = raw(enc, vals, off, w, dim, 0)              # (sizing, with planes given)
    assert rc == pkg.ERR_ARG and need == U
    rc, need, planes = raw(enc, vals, off, w, dim, U - 1)
    assert rc == pkg.ERR_ARG and need == U and all((p == CANARY).all() for p in planes)
    rc, need, planes = raw(enc, vals, off, w, dim, U)
    assert rc == 0 and need == U
    assert all((p[:PAD] == CANARY).all() and (p[PAD + U:] == CANARY).all() for p in planes)
    check([p[PAD:PAD + U] for p in planes], texts, w, dim)
    for kw in (dict(w=0), dict(w=WMAX + 1), dict(dim=0), dict(dim=MAX_DIM + 1), dict(off=off[::-1].copy()),
               dict(off=np.array([-1, 2], np.int64))):
        rc, need, planes = raw(enc, vals, kw.get('off', off), kw.get('w', w), kw.get('dim', dim), U)
        assert rc == pkg.ERR_ARG and all((p == CANARY).all() for p in planes), kw
    assert enc.skipgram_counts(vals[:0], np.zeros(1, np.int64), w, dim)[2].size == 0


def test_golden_cases_count_the_references_own_pairs(enc):
    """tests/golden/skipgram_cases.json: the pairs the reference's loop made, counted (its values ranked,
    to fit MAX_DIM), each window's cases as one batch."""
    with open(os.path.join(ROOT, 'tests', 'golden', 'skipgram_cases.json')) as f:
        cases = json.load(f)['cases']
    rank = {v: r for r, v in enumerate(sorted({v for c in cases for v in c['values']}))}
    dim = len(rank)
    for w in sorted({c['window'] for c in cases}):
        mine = [c for c in cases if c['window'] == w]
        want = collections.Counter((rank[a], rank[b]) for c in mine for a, b in c['pairs'])
        t, c, n = host_twice(enc, [[rank[v] for v in c['values']] for c in mine], w, dim)
        assert list(zip(t.tolist(), c.tolist())) == sorted(want) and n.tolist() == [want[k] for k in sorted(want)]


def test_text_and_utf8_forms_on_the_oracles_vectors():
    case = trained_case()
    e, _c = trained_encoder(case)
    try:
        dim = max(x for v in case['vectors'] for x in v) + 1
        for w in (1, 2, 5):
            a = e.skipgram_counts_text(case['samples'], w, 'vectors', dim)
            b = e.skipgram_counts_utf8([s.encode('utf-8') for s in case['samples']], None, w, 'vectors', dim)
            check(a, case['vectors'], w, dim)
            assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
        ids = e.encode_text(case['samples'], 'ids')
        check(e.skipgram_counts_text(case['samples'], 2, 'ids', 4096), ids, 2, 4096)
        with pytest.raises(pkg.BpeError, match=r'outside \[0, 3\) \(text \d+, position \d+\)'):
            e.skipgram_counts_text(case['samples'], 2, 'vectors', 3)
        bad = next(ch for ch in 'qzXQ~#☃' if ch not in _c.char_to_index)
        with pytest.raises(pkg.BpeError, match=r'unknown token, char: U\+%04X \(text 0, unit 0\)' % ord(bad)):
            e.skipgram_counts_utf8([bad.encode()], None, 2, 'vectors', dim)
    finally:
        e.close()


def test_corpus_forms_read_only_and_two_shards():
    e, done = trained_engine()
    twin, _ = trained_engine()
    multi, done2 = trained_engine(devices=[0, 0], reduce='host')
    try:
        assert len(done) == 12 and done2 == done and multi.shard_count() == 2
        tvi = full_index(e)
        for idx in (None, [3, 3, 1, 0, 3, 5, 5], []):
            for kind, index in (('ids', None), ('vectors', tvi)):
                vals, voff = e.export_samples(idx, kind, index)
                rows = [vals[voff[k]:voff[k + 1]] for k in range(len(voff) - 1)]
                for w in (1, 5):
                    got = check(e.export_skipgram_counts(idx, w, kind, None, index), rows, w, e.num_tokens())
                    two = multi.export_skipgram_counts(idx, w, kind, None, index)
                    assert all(x.tobytes() == y.tobytes() for x, y in zip(got, two)), (idx, kind, w)
        assert e.skipgram_counts_stats()['distinct_out'] > 100 and multi.skipgram_counts_stats()['distinct_out'] > 100
        with pytest.raises(pkg.BpeError, match=r'outside \[0, 2\) \(text 0, position \d+\)'):
            e.export_skipgram_counts(None, 2, 'ids', 2)
        need = ctypes.c_int64(-7)
        rc = pkg.lib().bpe_export_skipgram_counts_device(multi._ctx, pkg.EXPORT_IDS, None, len(CORPUS), None, 0, 2, 64,
                                                         None, None, None, 0, ctypes.byref(need))
        assert rc == pkg.ERR_ARG and need.value == -7 and 'multi-device' in pkg.last_error()
        # an export only reads: the next merges are those of the twin that never exported
        assert e.merge_until(0, 2, 30) == twin.merge_until(0, 2, 30)
    finally:
        for x in (e, twin, multi):
            x.close()


def device_form_check():
    """The tensor forms (the device forms) equal the restatement with the values at each of the four
    addresses mod 16; planes between canaries, capacity U - 1; text, UTF-8 and corpus equal the host's."""
    import torch
    dev = torch.device('cuda', 0)
    e = pkg.Encoder(0)
    batches = [edge_batch(2), edge_batch(WMAX), empties_batch(5), FIXED['overflow']]
    for n_b, (texts, w, dim) in enumerate(batches):
        for lead in range(4) if n_b == 0 else [1 + n_b % 3]:
            vals, off = flat(texts, lead=[-1] * lead)
            d_vals, d_off = torch.from_numpy(vals).to(dev), torch.from_numpy(off).to(dev)
            assert (d_vals.data_ptr() // 4 + lead) % 4 == lead
            got = e.skipgram_counts_tensors(d_vals, d_off, w, dim)
            assert all(x.is_cuda for x in got)
            check(got, texts, w, dim)
    U = got[0].numel()
    for cap, k0 in ((U - 1, 1), (U, 3), (U, 0)):
        bufs = [torch.full((U + 2 * PAD,), CANARY, dtype=dt, device=dev) for dt in (torch.int32, torch.int32, torch.int64)]
        views = [b[PAD + k0 + (j == 1):][:cap] for j, b in enumerate(bufs)]   # (the planes at addresses of their own)
        if cap < U:
            with pytest.raises(pkg.BpeError, match='need %d distinct pairs' % U):
                e.skipgram_counts_tensors(d_vals, d_off, w, dim, out=views)
            assert all((b == CANARY).all().item() for b in bufs)
        else:
            res = e.skipgram_counts_tensors(d_vals, d_off, w, dim, out=views)
            assert all(torch.equal(x, y) for x, y in zip(res, got))
            assert all((b == CANARY).sum().item() == 2 * PAD for b in bufs)
    e.close()
    case = trained_case()
    e, _c = trained_encoder(case)
    units, uoff = pkg._units_flat(case['samples'])
    data, boff = pkg._utf8_flat([s.encode('utf-8') for s in case['samples']], None)
    host = e.skipgram_counts_text(case['samples'], 3, 'vectors', 4096)
    for got in (e.skipgram_counts_text_tensors(torch.from_numpy(units.view(np.int16).copy()).to(dev),
                                               torch.from_numpy(uoff).to(dev), 3, 'vectors', 4096),
                e.skipgram_counts_utf8_tensors(torch.from_numpy(data.copy()).to(dev), torch.from_numpy(boff).to(dev), 3,
                                               'vectors', 4096)):
        assert len(host[0]) > 50 and all(np.array_equal(x.cpu().numpy(), y) for x, y in zip(got, host))
    e.close()
    eng, _done = trained_engine()
    host = eng.export_skipgram_counts(None, 2, 'vectors', None, full_index(eng))
    got = eng.export_skipgram_counts_tensors(None, 2, 'vectors', None, full_index(eng))
    assert len(host[0]) > 50 and all(np.array_equal(x.cpu().numpy(), y) for x, y in zip(got, host))
    eng.close()
    return True


def test_device_forms_equal_the_restatement_and_the_host_forms():
    """In a process of its own that imports torch before libbpe loads (PyTorch sees a device only
    when its HIP runtime is the process's first)."""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join(
        [here, os.path.join(os.path.dirname(here), 'oracle'), os.environ.get('PYTHONPATH', '')]))
    out = subprocess.run([sys.executable, os.path.abspath(__file__), 'device-form'], env=env,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith('device form ok'), \
        out.stdout[-2000:] + out.stderr[-3000:]


if __name__ == '__main__' and sys.argv[1:] == ['device-form']:
    import torch  # noqa: F401  (before libbpe loads)
    print('device form ok' if device_form_check() else 'failed')
